"""CPU tests of the one place every parameter-versioned cache goes through (normflows_amd._keys.cached / pcached): miss, hit, rebuild,
sub-slots, the states invalidate_caches leaves behind, the naming rule of the slots, and LULinearPermute._dense_matrices on top of it."""
import os

import pytest
import torch


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


class _Counter:
    """A `build` callable that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return ("value", self.n)


def test_miss_builds_hit_does_not_changed_key_rebuilds(nfa):
    keys, m, build = nfa._keys, torch.nn.Module(), _Counter()
    assert "_a_cache" not in m.__dict__
    v1 = keys.cached(m, "_a_cache", ("k", 1), build)
    assert build.n == 1 and v1 == ("value", 1)
    assert m.__dict__["_a_cache"] == (("k", 1), v1)                     # the stored format: (key, value)
    assert keys.cached(m, "_a_cache", ("k", 1), build) is v1 and build.n == 1      # an EQUAL key (another object) is a hit
    v2 = keys.cached(m, "_a_cache", ("k", 2), build)
    assert build.n == 2 and v2 == ("value", 2) and m.__dict__["_a_cache"] == (("k", 2), v2)
    assert keys.cached(m, "_a_cache", ("k", 1), build) == ("value", 3)  # one entry per slot: the old key is gone


def test_pcached_key_is_parameter_versions_then_extras(nfa):
    keys, m, build = nfa._keys, torch.nn.Module(), _Counter()
    p = torch.nn.Parameter(torch.zeros(3))
    keys.pcached(m, "_p_cache", [p], ("cpu", True), build)
    assert m.__dict__["_p_cache"][0] == keys.pkey([p]) + ("cpu", True)
    keys.pcached(m, "_p_cache", [p], ("cpu", True), build)
    assert build.n == 1
    keys.pcached(m, "_p_cache", [p], ("cpu", False), build)             # an extra changed
    assert build.n == 2
    with torch.no_grad():
        p.add_(1.0)                                                     # the parameter changed in place
    keys.pcached(m, "_p_cache", [p], ("cpu", False), build)
    assert build.n == 3


def test_sub_slots_are_independent(nfa):
    keys, m = nfa._keys, torch.nn.Module()
    a, b = _Counter(), _Counter()
    keys.cached(m, "_d_cache", "k", a, sub=None)                        # None is a sub like any other (the wide pack's own slot)
    keys.cached(m, "_d_cache", "k", b, sub=(1, 0))
    assert (a.n, b.n) == (1, 1)
    assert m.__dict__["_d_cache"] == {None: ("k", ("value", 1)), (1, 0): ("k", ("value", 1))}      # a dict of (key, value)
    keys.cached(m, "_d_cache", "k2", a, sub=None)                       # rebuilding one leaves the other
    keys.cached(m, "_d_cache", "k", b, sub=(1, 0))
    assert (a.n, b.n) == (2, 1)
    assert m.__dict__["_d_cache"][(1, 0)] == ("k", ("value", 1))


def test_what_invalidate_caches_leaves_is_a_miss(nfa):
    keys, m, build = nfa._keys, torch.nn.Module(), _Counter()
    m.__dict__["_a_cache"] = None                                       # a plain slot after invalidate_caches
    assert keys.cached(m, "_a_cache", "k", build) == ("value", 1)
    m.__dict__["_d_cache"] = None                                       # a dict slot that a test (or an older pickle) set to None
    assert keys.cached(m, "_d_cache", "k", build, sub=True) == ("value", 2)
    assert m.__dict__["_d_cache"] == {True: ("k", ("value", 2))}
    m.__dict__["_d_cache"] = ("k", object())                            # ... or to a tuple
    assert keys.cached(m, "_d_cache", "k", build, sub=True) == ("value", 3)
    assert m.__dict__["_d_cache"] == {True: ("k", ("value", 3))}
    m.__dict__["_a_cache"] = {}                                         # a plain slot holding the emptied dict
    assert keys.cached(m, "_a_cache", "k", build) == ("value", 4)


@pytest.mark.parametrize("slot", ["_pack", "cache", "_cache_x", "_structs", "_tcache"])
def test_slot_names_outside_the_rule_raise(nfa, slot):
    m, build = torch.nn.Module(), _Counter()
    with pytest.raises(AssertionError):
        nfa._keys.cached(m, slot, "k", build)
    with pytest.raises(AssertionError):
        nfa._keys.pcached(m, slot, [], (), build, sub=0)
    assert build.n == 0 and slot not in m.__dict__


def test_invalidate_caches_drops_cache_slots_and_keeps_struct_slots(nfa):
    keys = nfa._keys
    child = torch.nn.Module()
    root = torch.nn.ModuleList([child])
    build = _Counter()
    keys.cached(root, "_a_cache", "k", build)
    keys.cached(child, "_b_cache", "k", build)
    keys.cached(child, "_d_cache", "k", build, sub=0)
    keys.cached(child, "_d_cache", "k", build, sub=1)
    keys.cached(root, "_a_struct", "k", build)
    keys.cached(child, "_d_struct", "k", build, sub=0)
    structs = (root.__dict__["_a_struct"], dict(child.__dict__["_d_struct"]))
    nfa.invalidate_caches(root)
    assert root.__dict__["_a_cache"] is None and child.__dict__["_b_cache"] is None and child.__dict__["_d_cache"] == {}
    assert root.__dict__["_a_struct"] is structs[0] and child.__dict__["_d_struct"] == structs[1]
    n = build.n
    keys.cached(root, "_a_struct", "k", build)
    keys.cached(child, "_d_struct", "k", build, sub=0)
    assert build.n == n                                                 # the structures are still hits
    keys.cached(child, "_d_cache", "k", build, sub=0)
    assert build.n == n + 1                                             # the caches are rebuilt


def _lu(nfa, D, state=None):
    torch.manual_seed(D)
    lu = nfa.flows.LULinearPermute(D, identity_init=False)
    if state is not None:
        lu.load_state_dict(state, strict=True)
    return lu


@pytest.mark.parametrize("D", [5, 70])
def test_dense_matrices_follow_the_parameters(nfa, monkeypatch, D):
    """LULinearPermute._dense_matrices, one width per composer (D <= 64: ops.lu_compose, wider: _compose_wide): the same before and
    after invalidate_caches, and after an in-place update equal to what a fresh layer with that state composes.  nf_lu_compose is a
    device kernel (there is no CPU path), so for D = 5 the host test puts the float64 torch composer in its place -- the cache, not
    the composer's arithmetic, is under test here; tests/test_gpu_cache_keys.py runs both widths on the kernel."""
    calls = []
    real_wide = nfa.flows.LULinearPermute._compose_wide

    def lu_compose(perm, low, up, diag, bias, eps=1e-3):
        calls.append("lu_compose")
        twin = nfa.flows.LULinearPermute(bias.numel())
        twin.permutation._permutation.copy_(perm)
        with torch.no_grad():
            for p, v in zip((twin.linear.lower_entries, twin.linear.upper_entries, twin.linear.unconstrained_upper_diag,
                             twin.linear.bias), (low, up, diag, bias)):
                p.copy_(v)
        twin.linear.eps = eps
        return real_wide(twin)

    def compose_wide(self):
        calls.append("compose_wide")
        return real_wide(self)

    monkeypatch.setattr(nfa.ops, "lu_compose", lu_compose)
    monkeypatch.setattr(nfa.flows.LULinearPermute, "_compose_wide", compose_wide)
    lu = _lu(nfa, D)
    composer = "lu_compose" if D <= 64 else "compose_wide"
    m0 = lu._dense_matrices()
    assert calls == [composer] and len(m0) == 5 and m0[0].shape == (D, D)
    assert lu.__dict__["_dense_cache"][1] is m0
    assert lu._dense_matrices() is m0 and calls == [composer]           # a hit
    nfa.invalidate_caches(lu)
    assert lu.__dict__["_dense_cache"] is None
    m1 = lu._dense_matrices()
    assert calls == [composer] * 2 and all(torch.equal(a, b) for a, b in zip(m0, m1))
    with torch.no_grad():
        lu.linear.lower_entries.add_(0.1)
    m2 = lu._dense_matrices()
    assert calls == [composer] * 3 and not torch.equal(m2[0], m0[0])
    fresh = _lu(nfa, D, state=lu.state_dict())
    m3 = fresh._dense_matrices()
    assert len(m3) == 5 and all(torch.equal(a, b) for a, b in zip(m2, m3))
