"""CPU tests of tests/stream_kernel_cases.py, the case table behind tests/test_gpu_stream_kernels.py: the table holds every
(path, one sweep or more, full or ragged last sweep) cell the launchers can produce; its references are finite except at the entries
a case names; and the float32 yardstick stays within the bar each case will use, so that the bar is set by the kernel's arithmetic
and not by an ill-conditioned input."""
import pytest
import torch

import stream_kernel_cases as sc

KERNELS = sorted(sc.PATHS)


def case(kernel, dtype="f32", **p):
    return sc.plans(sc.Case(kernel, dtype, **p))


def test_grid_for_and_the_named_thresholds():
    """The shapes the table relies on for a later sweep, re-derived: each passes its cap by the stated number of rows."""
    assert sc.grid_for(1, 256) == 1 and sc.grid_for(0, 256) == 1 and sc.grid_for(10 ** 9, 256) == sc.CAP
    assert sc.grid_for(4097, 1, sc.CAP_IMG) == 4096
    pl = case("masked_affine", B=131137, inner=16, direction=0)["rows"]
    assert (pl.path, pl.sweeps, pl.per_sweep, 131137 - pl.per_sweep) == ("vec4/pow2", 2, 131072, 65)
    pl = case("masked_affine", B=103, inner=20, direction=0)["rows"]          # L4 = 5 of P = 8 lanes, 8 rows per wave, 3 workgroups
    assert (pl.path, pl.sweeps, pl.per_sweep) == ("vec4/idle-lanes", 2, 96)
    assert case("masked_affine", B=9, inner=132, direction=0)["rows"].path == "vec4/idle-lanes"
    assert case("masked_affine", "f64", B=50, inner=8, direction=0)["rows"].path == "short/pow2"
    pl = case("masked_affine", B=4099, inner=65, direction=0)["rows"]
    assert (pl.path, pl.sweeps, pl.per_sweep) == ("generic/one-pass", 2, 4096)
    assert case("masked_affine", B=3, inner=1030, direction=0)["rows"].path == "generic/thread-stride"
    pl = case("diag_gaussian", B=8197, d=5)["rows"]
    assert (pl.path, pl.sweeps, pl.per_sweep) == ("wave/one-pass", 2, 8192)
    assert case("diag_gaussian", "f64", B=70, d=128)["rows"].path == "wave/lane-stride"
    pl = case("affine_coupling", B=4099, C=3, c1=2, HW=1, smap="exp", flip=False, direction=0)["images"]
    assert (pl.sweeps, pl.per_sweep) == (2, 4096)
    pl = case("actnorm", B=2049, C=4, HW=256, direction=0)
    assert pl["elements"].sweeps == 5 and pl["elements"].per_sweep == 2048 * 256 and pl["ld-rows"].sweeps == 1
    assert case("actnorm", B=1500, C=1, HW=1, direction=0)["ld-rows"].sweeps == 3
    assert case("actnorm", B=1000, C=3, HW=1, direction=0)["ld-rows"].sweeps == 2
    pl = case("maf_affine_bwd", B=8070, D=65, direction=0)["elements"]
    assert (pl.sweeps, pl.per_sweep, 8070 * 65 - pl.per_sweep) == (2, 524288, 262)
    pl = case("squeeze", B=33, C=4, H=128, W=128, direction=0)["elements"]
    assert (pl.sweeps, pl.per_sweep) == (5, 2048 * 256)
    pl = case("ld_fold", B=524353, n=121, signs="flips")["rows"]
    assert (pl.path, pl.sweeps, 524353 - pl.per_sweep) == ("second-launch", 2, 65)
    pl = case("inv1x1_conv", B=4100, C=9, HW=64, variant="plain")
    assert (pl["pixels"].path, pl["pixels"].sweeps, pl["ld-rows"].sweeps) == ("4-loop+tail", 2, 1)
    assert case("inv1x1_conv", B=524353, C=1, HW=1, variant="plain")["ld-rows"].sweeps == 2
    pl = case("inv1x1_wgrad", B=600, C=17, HW=48)["chunks"]                   # the MFMA kernel stays in one sweep up to HW = 256 ...
    assert (pl.path, pl.sweeps) == ("mfma/NB=2", 1)
    pl = case("inv1x1_wgrad", B=1, C=17, HW=528)["chunks"]                    # ... and 33 chunks on one workgroup take three
    assert (pl.sweeps, pl.ragged) == (3, True)
    pl = case("inv1x1_wgrad", B=257, C=17, HW=15)["images"]                   # ipw = 2, the last workgroup holds one image
    assert (pl.path, pl.sweeps, pl.ragged) == ("partial/f32", 2, True)


def test_actnorm_bwd_carry_needs_a_second_image_in_a_later_sweep():
    """The shapes of HW = 12, 20, 36 with few channels leave one image (or one sweep) per workgroup: the (k, q) carry is computed and
    never used.  The table therefore holds C = 2048 shapes (nsplit = 1) whose workgroups walk several images over several sweeps."""
    for B, C, HW in ((100, 48, 12), (5, 3, 20), (700, 3, 36)):
        assert case("actnorm_bwd", B=B, C=C, HW=HW, direction=0)["walk"].sweeps == 1
    pl = case("actnorm_bwd", B=2, C=2, HW=1296, direction=0)["walk"]
    assert (pl.path, pl.sweeps) == ("quad/dk=0/one-image", 2)
    pl = case("actnorm_bwd", B=40, C=2048, HW=36, direction=0)["walk"]
    assert (pl.path, pl.sweeps, pl.ragged) == ("quad/carry/images>=2", 2, True)
    pl = case("actnorm_bwd", B=2, C=2048, HW=1028, direction=0)["walk"]
    assert (pl.path, pl.sweeps) == ("quad/dk=0/images>=2", 3)
    assert case("actnorm_bwd", "f64", B=50, C=2048, HW=12, direction=0)["walk"].path == "scalar/carry/images>=2"


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_reachable_cell_is_held(kernel):
    held = sc.cells(kernel)
    assert held, kernel
    for loop, path, multi, ragged in held:
        assert path in sc.PATHS[kernel][loop], (kernel, loop, path)
        assert (kernel, loop, path, multi, ragged) not in sc.UNREACHABLE, (kernel, loop, path, multi, ragged, held[loop, path, multi, ragged][0])
    missing = [(loop, path, multi, ragged) for loop, paths in sc.PATHS[kernel].items() for path in paths for multi in (False, True)
               for ragged in (False, True)
               if (loop, path, multi, ragged) not in held and (kernel, loop, path, multi, ragged) not in sc.UNREACHABLE]
    assert not missing, "%s: (loop, path, more than one sweep, ragged) cells without a case: %s" % (kernel, missing)
    for key, reason in sc.UNREACHABLE.items():
        assert key[0] in sc.PATHS and key[2] in sc.PATHS[key[0]][key[1]] and len(reason) > 20, key


def _small_shapes(kernel):
    """A brute-force sweep of small shapes through plans(): every workgroup count from one to a few, widths around every threshold."""
    two = ("f32", "f64")
    if kernel == "masked_affine":
        return [sc.Case(kernel, dt, B=B, inner=n, direction=0) for dt in two for B in range(1, 300) for n in (1, 2, 3, 4, 5, 8, 12, 16, 20,
                33, 63, 64, 65, 132, 256, 257, 260)] + [sc.Case(kernel, dt, B=B, inner=65, direction=0) for dt in two for B in (4096, 4097, 8192)]
    if kernel in ("affine_coupling", "affine_coupling_bwd"):
        return [sc.Case(kernel, dt, B=B, C=3, c1=1, HW=HW, smap="exp", flip=False, direction=0) for dt in two
                for B in list(range(1, 40)) + [4096, 4097, 8192] for HW in (1, 128, 129, 150)]
    if kernel == "actnorm":
        return [sc.Case(kernel, dt, B=B, C=C, HW=HW, direction=0) for dt in two for B in list(range(1, 40)) + list(range(250, 260)) +
                [512, 1024, 2048] for C in (1, 2, 3, 4, 5) for HW in (1, 2, 4, 5, 256)]
    if kernel == "actnorm_bwd":
        return [sc.Case(kernel, dt, B=B, C=C, HW=HW, direction=0) for dt in two for B in list(range(1, 20)) + [64, 128, 256, 300]
                for C in (1, 3, 1024, 2048) for HW in (1, 2, 3, 4, 6, 12, 16, 36, 64, 128, 256, 257, 300, 512, 1024, 1028, 1536)]
    if kernel == "inv1x1_wgrad":
        return [sc.Case(kernel, dt, B=B, C=C, HW=HW) for dt in two for B in list(range(1, 20)) + [255, 256, 257, 511, 512, 513, 600]
                for C in (1, 16, 17, 33, 49) for HW in (1, 15, 16, 48, 256, 272, 512)]
    return []


@pytest.mark.parametrize("kernel", sorted({k[0] for k in sc.UNREACHABLE}))
def test_no_small_shape_lands_in_a_cell_listed_as_unreachable(kernel):
    """UNREACHABLE is trusted by the coverage test above for every cell no case holds: here each kernel with such entries is swept
    over hundreds to thousands of small shapes, and none of them may land in a listed cell."""
    shapes = _small_shapes(kernel)
    assert len(shapes) > 300, kernel
    for c in shapes:
        for loop, pl in c.plans().items():
            assert (kernel, loop, pl.path, pl.sweeps > 1, pl.ragged) not in sc.UNREACHABLE, (c, loop, pl)


def test_every_kernel_takes_each_accumulator_mode_once():
    for kernel, kinds in sc.KIND.items():
        if ("ld" in kinds or "lp" in kinds) and not kernel.endswith("bwd") and kernel != "ld_fold":
            modes = {c.p.get("acc") for c in sc.CASES if c.kernel == kernel}
            assert {"write", "add", "sub"} <= modes, (kernel, modes)


@pytest.mark.parametrize("kernel", KERNELS)
def test_references_are_finite_and_yardsticks_within_their_bars(kernel):
    """Per case: the float64 reference is finite except at the named entries (whose NaN pattern the yardstick shares), and the float32
    yardstick's error, printed in units of the suite's existing bar, stays below YARD_LIMIT = 1: the plain float32 formula itself is
    inside the existing bar on every case, so a case's bar max(1, MARGIN x yardstick error) is at most MARGIN x the existing bar and
    no input is ill-conditioned.  (Measured: below 0.15 on every case, so the existing bars decide.)"""
    worst = {}
    for c in [c for c in sc.CASES if c.kernel == kernel]:
        x, ref, yard = c.evaluate()
        named = c.p.get("nonfinite") or c.p.get("bad_labels")
        for name, r in ref.items():
            assert r.dtype == torch.float64, (c, name)
            if not named:
                assert bool(torch.isfinite(r).all()), (c, name)
            else:
                assert 0 < int((~torch.isfinite(r)).sum()) <= 4 * max(1, r.numel() // c.p["B"]), (c, name)
            if yard is None:
                continue
            assert torch.equal(torch.isnan(yard[name]), torch.isnan(r)) and torch.equal(torch.isinf(yard[name]), torch.isinf(r)), (c, name)
            kind = sc.KIND[kernel][name]
            if kind == "exact":          # (held to the formula's own bits in the kernel's precision, not to a bar)
                assert yard[name].dtype == torch.float32
                continue
            e = sc.scaled_error(yard[name], r, kind, c.dtype)
            assert e <= YARD_LIMIT, "%s %s: the float32 formula itself is %.2f x the existing bar away from float64" % (c, name, e)
            worst[name] = max(worst.get(name, 0.0), e)
    print(kernel, "worst float32 yardstick error / existing bar:", {k: "%.3f" % v for k, v in worst.items()})


YARD_LIMIT = 1.0
