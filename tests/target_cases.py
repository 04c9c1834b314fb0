"""Cases of the target / prior / mixture fixtures, shared by tests/golden/make_golden_targets.py and the tests.

CASES_2D: name -> (class name, constructor arguments); 256 rows each, the first eight the edge rows below (the origin, the kinks at
z0 = 0 that float32 represents exactly, a far row), the rest 2.5 * randn.  Smiley's kink at z1 = -0.8 is not representable in
float32 and no row lies on it.  GMM: name -> (n_modes, dim); 200 rows of 3 * randn, row 0 set to 50 everywhere so that every mode
underflows against the maximum."""
import numpy as np
import torch

CASES_2D = {
    "two_moons": ("TwoMoons", ()),
    "two_modes_2_01": ("TwoModes", (2, 0.1)),
    "two_modes_m15_02": ("TwoModes", (-1.5, 0.2)),
    "sinusoidal": ("Sinusoidal", (0.4, 4)),
    "sinusoidal_gap": ("Sinusoidal_gap", (0.4, 4)),
    "sinusoidal_split": ("Sinusoidal_split", (0.4, 4)),
    "smiley": ("Smiley", (0.15,)),
    "ring_2": ("RingMixture", (2,)),
    "ring_3": ("RingMixture", (3,)),
    "circ_gmm_8": ("CircularGaussianMixture", (8,)),
    "circ_gmm_3": ("CircularGaussianMixture", (3,)),
}
EDGE_ROWS = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (2.0, 0.0), (-2.0, 0.0), (-0.0, 2.0), (1.0, 1e-20), (30.0, -30.0)]
KINK_ROWS = (0, 1, 5)          # rows exactly on a kink (z0 == 0 or the origin): compared with the reference's float32 leg
ROWS_2D = 256
SAMPLED = ("two_moons", "ring_2", "circ_gmm_8")      # cases with a seeded sample(n) in the fixture
N_SAMPLES = 64

GMM = {"m1_d2": (1, 2), "m3_d2": (3, 2), "m10_d2": (10, 2), "m5_d17": (5, 17), "m64_d64": (64, 64), "m7_d128": (7, 128)}
ROWS_GMM = 200


def build_2d(ns, name):
    """The instance of case `name` from namespace `ns` (an object with the classes as attributes)."""
    cls, args = CASES_2D[name]
    return getattr(ns, cls)(*args)


def rows_2d(seed):
    g = torch.Generator().manual_seed(seed)
    z = 2.5 * torch.randn(ROWS_2D, 2, generator=g)
    z[:len(EDGE_ROWS)] = torch.tensor(EDGE_ROWS)
    return z, torch.randn(ROWS_2D, generator=g)


def gmm_args(name, seed):
    """loc, scale, weights of a mixture case as numpy float64 arrays."""
    M, d = GMM[name]
    rs = np.random.RandomState(seed)
    return 2.0 * rs.randn(M, d), 0.5 + rs.rand(M, d), 0.2 + rs.rand(M)


def rows_gmm(name, seed):
    M, d = GMM[name]
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(ROWS_GMM, d, generator=g)
    z[0] = 50.0
    return z, torch.randn(ROWS_GMM, generator=g)
