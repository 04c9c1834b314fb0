#!/usr/bin/env python3
"""Records tests/golden/made_train_pack_parent.npz: sha1 digests of flows/made_pack.made_train_structure for three unpermuted MADEs
with an Identity preprocessing as the packer of ANOTHER revision of this package builds them -- the revision before _slot_layers /
_pack_backward_from learnt degree order (made_train_structure_ft).  Per case: table, src and the backward table, src, wtable, stable,
mask.  test_host_arnsf_train_ft.test_unpermuted_structures_unchanged compares this tree's arrays with them.
    git worktree add /tmp/before <revision before the change>
    python tests/golden/make_made_train_pack_parent.py /tmp/before
The packer is numpy on the CPU: no build and no GPU needed."""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("d6_h16_m2", 6, 16, 2), ("d32_h64_m23", 32, 64, 23), ("d128_h300_m2", 128, 300, 2))


def package(root):
    spec = importlib.util.spec_from_file_location("normflows_amd", os.path.join(root, "normalizing-flows_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["normflows_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def digests(nfa):
    from normflows_amd.flows import made_pack
    out = {}
    for name, D, H, mult in CASES:
        torch.manual_seed(7)
        made = nfa.nets.MADE(features=D, hidden_features=H, num_blocks=2, output_multiplier=mult)
        st = made_pack.made_train_structure(made, mult)
        arrays = {"table": st["table"], "src": st["src"]}
        arrays.update({"bwd_" + k: st["bwd"][k] for k in ("table", "src", "wtable", "stable", "mask")})
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            out["%s__%s" % (name, k)] = np.frombuffer(hashlib.sha1(str(a.dtype).encode() + a.tobytes()).digest(), dtype=np.uint8)
    return out


def main():
    nfa = package(os.path.abspath(sys.argv[1]))
    from normflows_amd.flows import made_pack
    assert not hasattr(made_pack, "made_train_structure_ft"), "this is the packer after the change: name a checkout of the revision before it"
    out = digests(nfa)
    np.savez_compressed(os.path.join(HERE, "made_train_pack_parent.npz"), **out)
    print("wrote made_train_pack_parent.npz: %s" % ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
