#!/usr/bin/env python3
"""Records tests/golden/arnsf_ft_pack_parent.npz: the per-feature AR packs (flows/maf_pack.pack_made(..., rows=True, features=...)) of
the three layers of tests/circ_wide_cases.ar_pack_cases as the packer of ANOTHER revision of this package writes them -- the revision
before maf_pack.feature_table was split into feature_rows + table_from_rows.  Per layer: the sha256 of blob, table and ftable, and the
ftable itself.  test_host_nsf_circ.test_ar_packs_unchanged_by_table_helper compares this tree's packs with them.
    git worktree add /tmp/before <revision before the split>
    python tests/golden/make_arnsf_ft_pack_parent.py /tmp/before
The packer is numpy on the CPU: no build and no GPU needed."""
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/: conftest, circ_wide_cases


def package(root):
    spec = importlib.util.spec_from_file_location("normflows_amd", os.path.join(root, "normalizing-flows_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["normflows_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    nfa = package(os.path.abspath(sys.argv[1]))
    import circ_wide_cases as cw
    from normflows_amd.flows import maf_pack
    assert not hasattr(maf_pack, "table_from_rows"), "this is the packer after the split: name a checkout of the revision before it"
    out = {}
    for name, t in cw.ar_pack_cases(nfa).items():
        packed = maf_pack.pack_made(t.autoregressive_net, mult=t._output_dim_multiplier(), rows=True, features=(t.tails, t.tail_bound))
        for part, a in zip(("blob", "table", "ftable"), packed):
            out["%s__%s_sha256" % (name, part)] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
        out[name + "__ftable"] = packed[2]
    np.savez_compressed(os.path.join(HERE, "arnsf_ft_pack_parent.npz"), **out)
    print("wrote arnsf_ft_pack_parent.npz: %s" % ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
