"""+-J graphs for the build matrix of the sparse kernels, made with numpy alone (no GPU, no library call), and the matrix itself:
the parameter lists of tests/test_gpu_pm1_builds.py, which tests/test_pm1_instances_cpu.py holds to the full cross products.

Graphs are (A, J): A[N, K] int32 with sorted rows, J[N, K] int8 in {-1, +1}, symmetric by construction (one draw per bond from a
seeded Generator, written at both ends)."""
import functools
import itertools

import numpy as np


def _couplings(A, seed):
    """One +-1 draw per bond x < y (in row order), stored at both ends."""
    N, K = A.shape
    rng = np.random.default_rng(seed)
    J = np.zeros((N, K), np.int8)
    pos = [{int(y): k for k, y in enumerate(A[x])} for x in range(N)]
    for x in range(N):
        for k in range(K):
            y = int(A[x, k])
            if x < y:
                j = 1 if rng.integers(0, 2) else -1
                J[x, k] = j
                J[y, pos[y][x]] = j
    assert (J != 0).all()
    return J


def complete(K, seed=0):
    """The complete graph on N = K + 1 sites: every closed neighbourhood is the whole graph, so every attempt of a chunk depends on the
    one before it (one slot per level, as many levels as the chunk is long), and N is below a wavefront."""
    N = K + 1
    A = np.array([[y for y in range(N) if y != x] for x in range(N)], np.int32)
    return A, _couplings(A, 1000 + 17 * K + seed)


def circulant(N, K, seed=0):
    """K-regular circulant graph: x ~ x +- 1 .. K // 2 and, for odd K, x + N / 2.  N >= 2 K + 2; N even when K is odd."""
    if N < 2 * K + 2 or (K % 2 and N % 2):
        raise ValueError("circulant(N=%d, K=%d): needs N >= 2 K + 2, and an even N for odd K" % (N, K))
    offs = [d for j in range(1, K // 2 + 1) for d in (j, -j)] + ([N // 2] if K % 2 else [])
    x = np.arange(N)[:, None]
    A = np.sort((x + np.array(offs)[None, :]) % N, axis=1).astype(np.int32)
    return A, _couplings(A, 2000 + 31 * N + K + seed)


def check_graph(A, J):
    """K-regular, simple, symmetric in A and in J."""
    N, K = A.shape
    assert A.min() >= 0 and A.max() < N
    assert (np.diff(A, axis=1) > 0).all() if K > 1 else True          # sorted rows, no double bond
    assert (A != np.arange(N)[:, None]).all()                         # no self-loop
    assert set(np.unique(J)) <= {-1, 1}
    D = {}
    for xx, yy, jj in zip(np.repeat(np.arange(N), K), A.reshape(-1), J.reshape(-1)):
        D[(int(xx), int(yy))] = int(jj)
    assert len(D) == N * K
    assert all(D.get((y, x_)) == j for (x_, y), j in D.items())


# ---- the matrix --------------------------------------------------------------------------------------------------------------------
KS = (1, 2, 3, 4, 5, 6, 7)
R = 33                                  # two replica groups, the second with one live replica
BETAS = (0.35, 1.2)                     # first call, second call: the threshold tables change between them

# path name -> (environment, the value rrrmc_sweep_layout reports)
PATHS = {
    "mode0":    ({"RRRMC_FORCE_WIDE": "0", "RRRMC_FORCE_SINGLE": "0", "RRRMC_FORCE_BIG": "0", "RRRMC_BIG_NO_MASKS": "0"}, 0),
    "mode1":    ({"RRRMC_FORCE_WIDE": "1", "RRRMC_FORCE_SINGLE": "0", "RRRMC_FORCE_BIG": "0", "RRRMC_BIG_NO_MASKS": "0"}, 1),
    "mode2":    ({"RRRMC_FORCE_WIDE": "2", "RRRMC_FORCE_SINGLE": "0", "RRRMC_FORCE_BIG": "0", "RRRMC_BIG_NO_MASKS": "0"}, 2),
    "mode3":    ({"RRRMC_FORCE_WIDE": "0", "RRRMC_FORCE_SINGLE": "1", "RRRMC_FORCE_BIG": "0", "RRRMC_BIG_NO_MASKS": "0"}, 3),
    "big":      ({"RRRMC_FORCE_WIDE": "0", "RRRMC_FORCE_SINGLE": "0", "RRRMC_FORCE_BIG": "1", "RRRMC_BIG_NO_MASKS": "0"}, 4),   # r = 32: four mask words
    "big_sweep": ({"RRRMC_FORCE_WIDE": "0", "RRRMC_FORCE_SINGLE": "0", "RRRMC_FORCE_BIG": "1", "RRRMC_BIG_NO_MASKS": "1"}, 6),
}
ENV_NAMES = ("RRRMC_FORCE_WIDE", "RRRMC_FORCE_SINGLE", "RRRMC_FORCE_BIG", "RRRMC_BIG_NO_MASKS", "RRRMC_BIG_LGR", "RRRMC_SWEEP_GENERIC")


def n200(K):
    return 202 if K % 2 else 200


def n201(K):
    """ragged last word of big_apply_kernel's LDS image for every S = 32 / r (201 and 202 are no multiples of 2 .. 32)"""
    return 202 if K % 2 else 201


@functools.lru_cache(maxsize=None)
def graph(shape):
    """shape: ("complete", K) | ("circulant", N, K) -> (A, J), built once and shared (read-only)"""
    A, J = complete(shape[1]) if shape[0] == "complete" else circulant(shape[1], shape[2])
    A.setflags(write=False)
    J.setflags(write=False)
    return A, J


def shapes_a(K):
    return (("complete", K), ("circulant", n200(K), K))


# (a) degree x path x shape
CASES_A = [(K, path, shape) for K in KS for path in PATHS for shape in shapes_a(K)]
# (b) long levels: the context's own layout and MODE 3 forced
CASES_B = [(K, forced) for K in KS for forced in (False, True)]
# (c) replicas per workgroup x degree on the big-N path
CASES_C = [(K, lgr) for K in KS for lgr in range(6)]
# (d) the size limit at natural size: ((L, D), no_masks)
CASES_D = [(LD, no_masks) for LD in ((1024, 2), (80, 3)) for no_masks in ("0", "1")]
# (e) colour sweeps
CASES_E = [(K, counting, shape) for K in KS for counting in (False, True) for shape in shapes_a(K)]
# (f) call shapes on every path: (iters, step) with "C" standing for the context's chunk length
CALL_SHAPES = ((1, 1), (5, 9), ("C", "C"), ("C+1", 1))
CASES_F = [(path, cs) for path in PATHS for cs in CALL_SHAPES]


def expected_products():
    """What the lists above must be: stated once more, independently, from the issue's cross products."""
    paths = ["mode0", "mode1", "mode2", "mode3", "big", "big_sweep"]
    a = [(K, p, s) for K, p, s in itertools.product(range(1, 8), paths, ("complete", "circulant"))]
    a = [(K, p, ("complete", K) if s == "complete" else ("circulant", 200 + 2 * (K % 2), K)) for K, p, s in a]
    e = [(K, c, ("complete", K) if s == "complete" else ("circulant", 200 + 2 * (K % 2), K))
         for K, c, s in itertools.product(range(1, 8), (False, True), ("complete", "circulant"))]
    return {
        "a": a,
        "b": list(itertools.product(range(1, 8), (False, True))),
        "c": list(itertools.product(range(1, 8), range(6))),
        "d": list(itertools.product(((1024, 2), (80, 3)), ("0", "1"))),
        "e": e,
        "f": list(itertools.product(paths, ((1, 1), (5, 9), ("C", "C"), ("C+1", 1)))),
    }


def big_path(K, lgr):
    """big_apply_kernel takes one compact mask word per (slot, workgroup) where the NT = (K + 1) / 2 classes' bits of its 2^lgr replicas
    fit one (DESIGN: lgr <= 4 and NT << lgr <= 32): path 5, else four words per (slot, group): path 4."""
    return 5 if lgr <= 4 and (((K + 1) // 2) << lgr) <= 32 else 4


def all_graph_shapes():
    """Every numpy-built graph shape the GPU matrix uses."""
    out = []
    for K in KS:
        for s in (("complete", K), ("circulant", n200(K), K), ("circulant", n201(K), K), ("circulant", 9000, K)):
            if s not in out:
                out.append(s)
    return out
