"""Plain numpy / Python restatement of the cross-replica overlaps (rrrmc_cross_overlaps, rrrmc_overlap_hist, parsexovs,
overlap_moments), from 0/1 arrays as ``Config.bits()`` gives them ([R, N]).  Everything is exact integer arithmetic, or Float64 in the
reference's own order of operations (scripts/scripts.jl:407-457)."""
import math

import numpy as np


def cross_matrix(bitsA, bitsB, N):
    """q[i, j] = pm1dot(A[i], B[j]) = N - 2 |A[i] xor B[j]| (scripts/scripts.jl:283-295)"""
    a = np.asarray(bitsA, np.int64)[:, :N]
    b = np.asarray(bitsB, np.int64)[:, :N]
    ham = a @ (1 - b).T + (1 - a) @ b.T
    return (N - 2 * ham).astype(np.int64)


def counted(same_slot, r1, r2):
    """a pair of one slot with itself counts each unordered pair of distinct replicas once, two different slots every r1 != r2"""
    return r1 < r2 if same_slot else r1 != r2


def hist(pairs, N):
    """pairs: a list of (bitsA, bitsB, same_slot); h[d] = the number of counted replica pairs at Hamming distance d, over all of them"""
    h = np.zeros(N + 1, np.int64)
    for bitsA, bitsB, same in pairs:
        q = cross_matrix(bitsA, bitsB, N)
        for r1 in range(q.shape[0]):
            for r2 in range(q.shape[1]):
                if counted(same, r1, r2):
                    h[(N - int(q[r1, r2])) // 2] += 1
    return h


def get_ts_range(ts, t0):
    i = next((k for k, t in enumerate(ts) if t >= t0), None)
    j = next((k for k, t in enumerate(ts) if t >= 2 * t0), None)
    return i, j


def pm1dot_cols(c1, c2, N):
    """pm1dot of two 0/1 columns"""
    return N - 2 * int(np.count_nonzero(np.asarray(c1) != np.asarray(c2)))


def parsexovs(cols1, cols2, ts1, ts2, lr):
    """scripts/scripts.jl:407-457 line for line; cols1 / cols2: [N, samples] 0/1 matrices (``SnapshotLog.to_mat``), 0-based ranges"""
    N, l1 = cols1.shape
    l2 = cols2.shape[1]
    assert cols2.shape[0] == N
    mx2s, sx2s = [], []
    for t_st in lr:
        i1, j1 = get_ts_range(ts1, t_st)
        i2, j2 = get_ts_range(ts2, t_st)
        if i1 is None or i2 is None:
            break
        if j1 is None:
            j1 = len(ts1)
        if j2 is None:
            j2 = len(ts2)
        mx2 = 0.0
        mx4 = 0.0
        n = 0
        for k1 in range(i1, j1):
            for k2 in range(i2, j2):
                x = pm1dot_cols(cols1[:, k1], cols2[:, k2], N) / N
                x2 = x * x                                  # Julia's x^2 is x * x (Base.literal_pow)
                mx2 += x2
                mx4 += x2 * x2
                n += 1
        mx2 = mx2 / n if n else float("nan")                # 0.0 / 0
        mx4 = mx4 / n if n else float("nan")
        d = mx4 - mx2 * mx2
        sx2 = float("nan") if math.isnan(d) else math.sqrt(max(0.0, d))        # Julia's max(0.0, NaN) is NaN
        mx2s.append(mx2)
        sx2s.append(sx2)
    return mx2s, sx2s


def moments(qs, N):
    """direct summation over a list of integer overlaps q: pairs, <q^2>, <q^4>, <|q|> of q / N and the Binder ratio"""
    qs = [int(q) for q in qs]
    n = len(qs)
    nan = float("nan")
    if n == 0:
        return {"pairs": 0, "q2": nan, "q4": nan, "binder": nan, "absq": nan}
    s1 = sum(abs(q) for q in qs)
    s2 = sum(q ** 2 for q in qs)
    s4 = sum(q ** 4 for q in qs)
    return {"pairs": n, "q2": s2 / (n * N ** 2), "q4": s4 / (n * N ** 4), "absq": s1 / (n * N),
            "binder": 0.5 * (3.0 - (s4 * n) / (s2 * s2)) if s2 else nan}
