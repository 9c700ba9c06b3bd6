"""One table of instances that sit on the size limits the library accepts, and on both sides of the rule that decides between the
LDS-resident and the global-memory build of a kernel.  tests/test_limit_instances_cpu.py holds every entry to its claims with the
plain-Python references alone; tests/test_gpu_limits.py runs every entry on the device against the same reference results.

An entry is an ``Entry``: a name, the family, the bounds it sits on — ``(what, literal, header constant)``, the literal written out here and
the constant named beside it — how to build the graph (``spec``), and the run: β, iterations per call, step, R, seed, sampler and, for
rrrMC, ``thr`` (staged_thr: 0.0 takes the direct branch only, 1.5 the staged branch only).  Every run is two consecutive calls, the second
continuing the random streams (``it0 = iters``).  ``build`` is the value the family's build reporter must give with no switch set (None:
the family has no reporter or one build), ``env`` the switches to set, ``lds`` the LDS bytes the host's formula gives for the shape.

Inputs are seeded (the library's host-only generators) or built here with numpy; nothing is read from a file.  The accepted counts beside
the entries are those of the reference (replica 0 .. R-1, first call / second call)."""
import collections
import functools

import numpy as np

import add_fields_reference as AF
import comm_reference as CR
import le_reference as LE
import perc_reference as PR
import quant_pattern_reference as QP
import re_reference as RE
import sat_reference as SR
import sparse_slice_reference as SP
import xentr_reference as XR

Entry = collections.namedtuple("Entry", "name family bounds spec run build env lds")

KLDS_LIMIT = 160 * 1024                  # kLdsLimit (rrrmc_hip.hip)
LDS, GLOBAL = 1, 2


def _run(beta, iters, step=None, R=3, seed=20261, sampler="std", thr=None):
    return dict(beta=beta, iters=iters, step=step or iters // 4, R=R, seed=seed, sampler=sampler, thr=thr)


def _e(name, family, bounds, spec, run, build=None, env=None, lds=None):
    return Entry(name, family, tuple(bounds), spec, run, build, dict(env or {}), lds)


# ---- the host's LDS formulas, restated (re_kernels.hpp:466, le_kernels.hpp:169, perc_kernels.hpp:64, af_kernels.hpp:50) --------------------
def _a4(x):
    return (x + 3) & ~3


def _a8(x):
    return (x + 7) & ~7


def _spin_words(N):
    return 2 * ((N + 63) // 64)


def re_lds_bytes(Nk, M, PW=0):
    """re_rrr_lds_bytes(N, W, Nk) and, over perceptron slices, the 8-byte aligned perc_lds_bytes(M, PW) behind it (host_re.hpp:112-113)"""
    N = Nk * M
    b = _spin_words(N) * 4 + _a4(2 * N) + _a4(N) + _a4(Nk) + 32 * 4 + 64 * 8 * 4
    return _a8(b) + M * PW * (2 * 8 + 64 * 2) if PW else b


def le_lds_bytes(Nk, M, PW=0):
    """le_rrr_lds_bytes and perc_lds_bytes(M + 1, PW) (host_le.hpp:144-145)"""
    N = Nk * (M + 1)
    b = _spin_words(N) * 4 + _a4(2 * N) + _a4(N) + _a4(Nk) + 2 * 17 * 4 + 64 * 8 * 4
    return _a8(b) + (M + 1) * PW * (2 * 8 + 64 * 2) if PW else b


def af_lds_bytes(N):
    """af_lds_bytes(N, N2, W) rounded up to 8 (host_af.hpp:190): the tree and the weights (16 N2), ΔEs (8 N), the spins"""
    N2 = 1
    while N2 < N:
        N2 *= 2
    return _a8(N2 * 16 + N * 8 + _a8(_spin_words(N) * 4))


# ---- the table --------------------------------------------------------------------------------------------------------------------------
PERC_N = ("N", 32767, "kPercNmax")
PERC_P = ("P", 4096, "kPercPmax")
ENS_N = ("N", 65535, "the ensembles' N <= 65535 (host_ens.hpp)")
AF_N = ("N", 65535, "kAfNmax")

ENTRIES = []

# GraphPercStep / GraphPercLinear under standardMC.  (N, P) on both bounds, each alone, and P in {4032, 4033, 4095}: the last mask word
# full, one bit into it, one bit short of it.  "start": "margin" puts every chain on a configuration where pattern 0 has Δ = +1 (a random
# start has |Δ| ~ sqrt(N) and a single pattern would never reach the p / m sets).
for _lin, _tag in ((False, "step"), (True, "linear")):
    ENTRIES += [
        # accepted step: [29, 33, 43] / [20, 13, 4]; linear: [243, 242, 256] / [258, 244, 250]
        _e("perc_%s_N32767_P4096" % _tag, "perc", [PERC_N, PERC_P], dict(linear=_lin, N=32767, P=4096, seed=771), _run(1.1, 300)),
        # accepted step at β = 3: [27, 21, 22] / [10, 2, 21]; linear at β = 40: [157, 140, 147] / [157, 154, 139]
        _e("perc_%s_N32767_P4096_cold" % _tag, "perc", [PERC_N, PERC_P], dict(linear=_lin, N=32767, P=4096, seed=771), _run(40.0 if _lin else 3.0, 300)),
        _e("perc_%s_N32767_P1" % _tag, "perc", [PERC_N, ("P", 1, "the least P")], dict(linear=_lin, N=32767, P=1, seed=772, start="margin"),
           _run(60.0 if _lin else 3.0, 300, seed=20293)),
        _e("perc_%s_N1_P4096" % _tag, "perc", [("N", 1, "the least N"), PERC_P], dict(linear=_lin, N=1, P=4096, seed=773), _run(0.01 if _lin else 0.02, 300)),
        _e("perc_%s_N3_P4095" % _tag, "perc", [("P", 4095, "kPercPmax - 1")], dict(linear=_lin, N=3, P=4095, seed=774), _run(0.02 if _lin else 0.03, 300)),
        _e("perc_%s_N101_P4032" % _tag, "perc", [("P", 4032, "63 full mask words")], dict(linear=_lin, N=101, P=4032, seed=775), _run(0.15 if _lin else 0.2, 600)),
        _e("perc_%s_N101_P4033" % _tag, "perc", [("P", 4033, "one bit into mask word 64")], dict(linear=_lin, N=101, P=4033, seed=776), _run(0.15 if _lin else 0.2, 600)),
    ]
# the crafted graphs (from_patterns): every chain starts on the configuration c; patterns equal to c have Δ = +32767, its complements
# Δ = -32767, the two ends of an int16.
# Nothing within reach of Δ = ±1 would leave the p / m sets empty for ever (and every ΔE of the step graph zero), so 8 patterns of one
# half are replaced by patterns at Δ = +1 (c with 16383 seeded bits flipped):
#   linear: 2040 at +32767, 2048 at -32767, 8 at +1: energy 2 * 2048 * 16384 / sqrt(N) exactly.  Every flip lowers the energy by about
#     2 * 2048 / sqrt(N) = 22.6: the run is made to decide by a negative β (acceptance exp(-1.13) = 0.32)
#   step: 2048 at +32767, 2040 at -32767, 8 at +1, energy 2040
ENTRIES += [
    _e("perc_step_crafted_int16_ends", "perc", [PERC_N, PERC_P, ("max Δ", 32767, "int16"), ("min Δ", -32767, "int16")],
       dict(linear=False, N=32767, P=4096, seed=777, crafted=(2048, 2040, 8), start="crafted"), _run(0.15, 300)),
    _e("perc_linear_crafted_int16_ends", "perc", [PERC_N, PERC_P, ("max Δ", 32767, "int16"), ("min Δ", -32767, "int16")],
       dict(linear=True, N=32767, P=4096, seed=777, crafted=(2040, 2048, 8), start="crafted"), _run(-0.05, 300)),
]

# GraphPercXEntr(32767, 4096, λ = 1) under standardMC in each build the switches select (rrrmc_xentr_build: 1 thread per chain, 2 wavefront
# per chain).  The loss table (N + 1 = 32768 doubles, 256 KiB) is beyond LDS in every one of them; the library computes it on the host and
# the reference is handed the same table.  One reference run serves the three entries.
XENTR_BUILDS = (("wave", {"RRRMC_XENTR_WAVE": "1"}, 2), ("thread", {"RRRMC_XENTR_NO_WAVE": "1"}, 1), ("no_lds", {"RRRMC_XENTR_NO_LDS": "1"}, 2))
ENTRIES += [
    _e("xentr_N32767_P4096_%s" % _tag, "xentr", [PERC_N, PERC_P, ("table entries", 32768, "N + 1")], dict(N=32767, P=4096, lam=1.0, seed=780, same_as="xentr_N32767_P4096_wave"),
       _run(1.0, 300, seed=20286), build=_bd, env=_env)
    for _tag, _env, _bd in XENTR_BUILDS]

# The Robust Ensemble and the Local Entropy ensemble.  N = Nk M (RE) or Nk (M + 1) (LE) = 65535 = 15 * 4369 = 17 * 3855 exactly; M on its
# bound (32 / 31) with the largest Nk that keeps N <= 65535 (2047 * 32 = 65504).  At these sizes the chain's hot state (3 N bytes and
# more) is beyond 160 KiB: the global-memory build.
for _ens, _rows, _Mmax in (("re", 0, ("M", 32, "kReMmax")), ("le", 1, ("M", 31, "kLeMmax"))):
    for _M1, _Nk in ((15, 4369), (17, 3855)):
        _M = _M1 - _rows
        ENTRIES += [
            _e("%s_empty_M%d_N65535_%s" % (_ens, _M, _s), _ens, [ENS_N], dict(slice="empty", Nk=_Nk, M=_M, gamma=1.0, beta_g=1.0),
               _run(1.5, 1000, sampler=_s, thr=_t, seed=20262 + _M), build=GLOBAL if _s != "std" else None,
               lds=(re_lds_bytes if _ens == "re" else le_lds_bytes)(_Nk, _M))
            for _s, _t in (("rrr_direct", 0.0), ("rrr_staged", 1.5), ("std", None))]
    _M = _Mmax[1]
    ENTRIES += [
        _e("%s_empty_M%d_Nk2047_%s" % (_ens, _M, _s), _ens, [_Mmax, ("N", 65504, "the largest multiple of 32 <= 65535")],
           dict(slice="empty", Nk=2047, M=_M, gamma=0.5, beta_g=1.0), _run(1.5, 1000, sampler=_s, thr=_t, seed=20270), build=GLOBAL if _s != "std" else None,
           lds=(re_lds_bytes if _ens == "re" else le_lds_bytes)(2047, _M))
        for _s, _t in (("rrr", 0.5), ("std", None))]

# ... and over perceptron slices at the same N (P = 65: a second mask word of one pattern), where rrrMC has a residual to accept or reject
ENTRIES += [
    _e("re_percstep_M15_N65535_%s" % _s, "re", [ENS_N], dict(slice="perc", linear=False, Nk=4369, P=65, M=15, gamma=1.0, beta_g=1.0, seed=781),
       _run(1.0, 600, sampler=_s, thr=_t, seed=20287), build=GLOBAL if _s != "std" else None, lds=re_lds_bytes(4369, 15, 2))
    for _s, _t in (("rrr", 0.5), ("std", None))]
ENTRIES += [
    _e("le_perclinear_M14_N65535_%s" % _s, "le", [ENS_N], dict(slice="perc", linear=True, Nk=4369, P=65, M=14, gamma=1.0, beta_g=1.0, seed=782),
       _run(3.0, 600, sampler=_s, thr=_t, seed=20288), build=GLOBAL if _s != "std" else None, lds=le_lds_bytes(4369, 14, 2))
    for _s, _t in (("rrr", 0.5), ("std", None))]

# ... over perceptron slices with P = 4096 at the same N, and over GraphSAT(4369, 3, 4.2) slices
ENTRIES += [
    _e("re_percstep_P4096_M15_N65535_rrr", "re", [ENS_N, PERC_P], dict(slice="perc", linear=False, Nk=4369, P=4096, M=15, gamma=1.0, beta_g=1.0, seed=783),
       _run(1.0, 300, sampler="rrr", thr=0.5, seed=20289), build=GLOBAL, lds=re_lds_bytes(4369, 15, 64)),
    _e("le_perclinear_P4096_M14_N65535_rrr", "le", [ENS_N, PERC_P], dict(slice="perc", linear=True, Nk=4369, P=4096, M=14, gamma=1.0, beta_g=1.0, seed=784),
       _run(1.0, 300, sampler="rrr", thr=0.5, seed=20290), build=GLOBAL, lds=le_lds_bytes(4369, 14, 64)),
    _e("re_sat_M15_N65535_rrr", "re", [ENS_N], dict(slice="sat", Nk=4369, K=3, alpha=4.2, M=15, gamma=1.0, beta_g=1.0, seed=785),
       _run(1.5, 1000, sampler="rrr", thr=0.5, seed=20294), build=GLOBAL, lds=re_lds_bytes(4369, 15)),
    _e("le_sat_M14_N65535_rrr", "le", [ENS_N], dict(slice="sat", Nk=4369, K=3, alpha=4.2, M=14, gamma=1.0, beta_g=1.0, seed=786),
       _run(1.5, 1000, sampler="rrr", thr=0.5, seed=20295), build=GLOBAL, lds=le_lds_bytes(4369, 14)),
]

# GraphCommStep (odd factors) and GraphCommReLU (even factors) under standardMC at the largest admissible K1 K2 in both orientations, with
# P = 64 (one mask word: the plain reference's work is P K2 per move), and P = 4096 at K1 = K2 = 21 / 20.  The reference is CommVec below.
COMM_N = ("N", 32767, "kCommNmax")
ENTRIES += [
    _e("commstep_K4681x7_P64", "comm", [COMM_N], dict(relu=False, K1=4681, K2=7, P=64, seed=790), _run(1.0, 600, seed=20301)),
    _e("commstep_K7x4681_P64", "comm", [COMM_N, ("K2", 4681, "the most units at odd K1 > 1 ... K1 = 7")], dict(relu=False, K1=7, K2=4681, P=64, seed=791), _run(1.0, 600, seed=20302)),
    _e("commrelu_K16382x2_P64", "comm", [("N", 32764, "the largest even x even product <= kCommNmax at K2 = 2")], dict(relu=True, K1=16382, K2=2, P=64, seed=792), _run(1.0, 600, seed=20303)),
    _e("commrelu_K2x16382_P64", "comm", [("N", 32764, "the largest even x even product <= kCommNmax at K1 = 2")], dict(relu=True, K1=2, K2=16382, P=64, seed=793), _run(1.0, 600, seed=20304)),
    _e("commstep_K21x21_P4096", "comm", [("P", 4096, "kCommPmax")], dict(relu=False, K1=21, K2=21, P=4096, seed=794), _run(0.3, 600, seed=20305)),
    _e("commrelu_K20x20_P4096", "comm", [("P", 4096, "kCommPmax")], dict(relu=True, K1=20, K2=20, P=4096, seed=795), _run(0.3, 600, seed=20306)),
    # GraphCommQu: Δ2 = o Σ_k c_k Δ1_k^2 in an int32.  At K2 = 2 (c = +1, -1) its largest magnitude is K1^2 = 16382^2 = 268 369 924 — the
    # crafted entry puts pattern 0 (label 1) and pattern 1 (label 0) there: unit 0 aligned with the start configuration, unit 1 balanced
    _e("commqu_K16382x2_P64", "comm", [("N", 32764, "the largest even x even product <= kCommNmax at K2 = 2")], dict(qu=True, relu=True, K1=16382, K2=2, P=64, seed=796), _run(1.0, 600, seed=20307)),
    _e("commqu_K2x16382_P64", "comm", [("N", 32764, "the largest even x even product <= kCommNmax at K1 = 2")], dict(qu=True, relu=True, K1=2, K2=16382, P=64, seed=797), _run(1.0, 600, seed=20308)),
    _e("commqu_K20x20_P4096", "comm", [("P", 4096, "kCommPmax")], dict(qu=True, relu=True, K1=20, K2=20, P=4096, seed=798), _run(0.3, 600, seed=20309)),
    _e("commqu_crafted_delta2_ends", "comm", [("max Δ2", 268369924, "K1^2 at K1 = 16382, in an int32"), ("min Δ2", -268369924, "-K1^2")],
       dict(qu=True, relu=True, K1=16382, K2=2, P=64, seed=799, crafted_qu=True, start="crafted_qu"), _run(1.0, 600, seed=20310)),
]

# RE / LE over binary GraphSK slices at N = 65535: a dense Nk x Nk coupling matrix under 16-bit set members (reference: SliceSKLean below)
ENTRIES += [
    _e("re_sk_M15_N65535_rrr", "re", [ENS_N], dict(slice="sk", Nk=4369, M=15, gamma=1.0, beta_g=1.0, seed=802), _run(1.0, 600, sampler="rrr", thr=0.5, seed=20313),
       build=GLOBAL, lds=re_lds_bytes(4369, 15)),
    _e("re_sk_M17_N65535_std", "re", [ENS_N], dict(slice="sk", Nk=3855, M=17, gamma=1.0, beta_g=1.0, seed=803), _run(1.0, 600, seed=20314)),
    _e("le_sk_M14_N65535_rrr", "le", [ENS_N], dict(slice="sk", Nk=4369, M=14, gamma=1.0, beta_g=1.0, seed=804), _run(1.0, 600, sampler="rrr", thr=0.5, seed=20315),
       build=GLOBAL, lds=le_lds_bytes(4369, 14)),
    _e("le_sk_M16_N65535_std", "le", [ENS_N], dict(slice="sk", Nk=3855, M=16, gamma=1.0, beta_g=1.0, seed=805), _run(1.0, 600, seed=20316)),
]

# GraphSAT under standardMC in the wavefront-per-replica build and, with RRRMC_SAT_NO_WAVE=1, the thread-per-replica build (rrrmc_sat_build:
# 1 thread, 2 wave); one reference run serves both.  N = 65535 at K = 3 (variable ids up to 65534 in 16 bits); N = 9 with 65535 clauses of
# 8 literals that all hold variable 0 (|T[0]| = 65535, one attempt in nine lands on it); exactly 2^20 clauses at N = 65535.
SAT_N = ("N", 65535, "kSatNmax")
# (sat_degree65535_thread takes about 15 s on the device and the 2^20-clause entries 8 to 10 s, at the floor of 300 iterations and whatever
# R is: in the thread build ONE thread walks the 57 000 to 65 535 clauses of the attempted variable, 8 literals each, at every one of the
# 600 attempts — that serial walk at |T[i]| = 65535 is what the entry is there to run — and the 2^20-clause graph and its reference take
# that long to build on the host.  The shapes are the issue's; the time is accepted.)
SAT_DEGREE_BETA = 0.02          # accepted: [262, 253, 239] / [249, 258, 253] of 300
for _tag, _env, _bd in (("wave", {}, 2), ("thread", {"RRRMC_SAT_NO_WAVE": "1"}, 1)):
    ENTRIES += [
        _e("sat_N65535_K3_%s" % _tag, "sat", [SAT_N, ("largest variable id", 65534, "uint16")], dict(kind="random", N=65535, K=3, alpha=4.2, seed=787, same_as="sat_N65535_K3_wave"),
           _run(2.0, 1000, seed=20296), build=_bd, env=_env),
        _e("sat_degree65535_%s" % _tag, "sat", [("max occurrences", 65535, "kSatDegMax"), ("literals", 8, "kSatLenMax")], dict(kind="degree", N=9, seed=788, same_as="sat_degree65535_wave"),
           _run(SAT_DEGREE_BETA, 300, seed=20297), build=_bd, env=_env),
        _e("sat_N65535_2p20_clauses_%s" % _tag, "sat", [SAT_N, ("clauses", 1048576, "kSatMcMax")], dict(kind="random", N=65535, K=3, alpha=1048576 / 65535, seed=789, same_as="sat_N65535_2p20_clauses_wave"),
           _run(0.5, 300, R=2, seed=20298), build=_bd, env=_env),
    ]

# GraphAddFields / GraphAddSubFields over GraphSAT(65535, 3, 4.2) and over GraphPercStep(32767, 4096): the residual is g's ΔE, rrrMC rejects
ENTRIES += [
    _e("af%d_sat_N65535_rrr" % _sub, "af", [AF_N, SAT_N], dict(sub=_sub, N=65535, g="sat", K=3, alpha=4.2, seed=787), _run(1.0, 1000, sampler="rrr", thr=0.5, seed=20299),
       build=GLOBAL, lds=af_lds_bytes(65535)) for _sub in (0, 1)]
ENTRIES += [
    _e("af%d_percstep_N32767_P4096_rrr" % _sub, "af", [PERC_N, PERC_P], dict(sub=_sub, N=32767, g="perc", P=4096, seed=771), _run(1.0, 300, sampler="rrr", thr=0.5, seed=20300),
       build=GLOBAL) for _sub in (0, 1)]

# GraphAddFields / GraphAddSubFields over GraphEmpty at N = 65535: a tree of 16 levels
for _sub in (0, 1):
    ENTRIES += [
        _e("af%d_empty_N65535_%s" % (_sub, _s), "af", [AF_N, ("tree levels", 16, "ceil(log2 N)")], dict(sub=_sub, N=65535), _run(1.0, 1000, sampler=_s, thr=_t, seed=20280),
           build=GLOBAL, lds=af_lds_bytes(65535))
        for _s, _t in (("rrr_direct", 0.0), ("rrr_staged", 1.5))]

# ---- the LDS-fit rule crossed by size: (largest shape the rule admits, the next admissible one), no switch set --------------------------
# Derived by hand from the formulas above; 160 KiB = 163840 bytes.
#   field wrappers over GraphEmpty, by N:  N = 4096: N2 = 4096, 65536 + 32768 + 512 = 98816;  N = 4097: N2 = 8192, 131072 + 32776 + 520 = 164368
#   RE over GraphEmpty, M = 3, by Nk:      Nk = 15581 (N = 46743): 5848 + 93488 + 46744 + 15584 + 128 + 2048 = 163840 (the limit itself);
#                                          Nk = 15582 (N = 46746): 5848 + 93492 + 46748 + 15584 + 128 + 2048 = 163848
#   LE over GraphEmpty, M = 3, by Nk:      Nk = 11974 (N = 47896): 5992 + 95792 + 47896 + 11976 + 136 + 2048 = 163840 (the limit itself);
#                                          Nk = 11975 (N = 47900): 5992 + 95800 + 47900 + 11976 + 136 + 2048 = 163852
#   RE over GraphPercStep(3, 4096), by M:  M = 17 (N = 51): 2344 + 17 * 64 * 144 = 159016;  M = 18 (N = 54): 2352 + 18 * 9216 = 168240
#   LE over GraphPercStep(3, 4096), by M:  M = 16 (17 rows, N = 51): 2352 + 17 * 9216 = 159024;  M = 17 (18 rows): 2360 + 18 * 9216 = 168248
PAIRS = []


def _pair(a, b):
    ENTRIES.extend([a, b])
    PAIRS.append((a.name, b.name))


for _sub in (0, 1):
    _pair(*[_e("af%d_empty_N%d_pair" % (_sub, _N), "af", [("LDS bytes", _b, "af_lds_bytes vs kLdsLimit = 163840")], dict(sub=_sub, N=_N),
               _run(1.0, 1000, sampler="rrr", thr=0.5, seed=20281), build=_bd, lds=_b) for _N, _b, _bd in ((4096, 98816, LDS), (4097, 164368, GLOBAL))])
_pair(*[_e("re_empty_M3_Nk%d_pair" % _Nk, "re", [("LDS bytes", _b, "re_rrr_lds_bytes vs kLdsLimit = 163840")], dict(slice="empty", Nk=_Nk, M=3, gamma=1.0, beta_g=1.0),
           _run(1.5, 1000, sampler="rrr", thr=0.5, seed=20282), build=_bd, lds=_b) for _Nk, _b, _bd in ((15581, 163840, LDS), (15582, 163848, GLOBAL))])
_pair(*[_e("le_empty_M3_Nk%d_pair" % _Nk, "le", [("LDS bytes", _b, "le_rrr_lds_bytes vs kLdsLimit = 163840")], dict(slice="empty", Nk=_Nk, M=3, gamma=1.0, beta_g=1.0),
           _run(1.5, 1000, sampler="rrr", thr=0.5, seed=20283), build=_bd, lds=_b) for _Nk, _b, _bd in ((11974, 163840, LDS), (11975, 163852, GLOBAL))])
_pair(*[_e("re_percstep_P4096_M%d_pair" % _M, "re", [PERC_P, ("LDS bytes", _b, "re_rrr_lds_bytes + perc_lds_bytes vs kLdsLimit = 163840")],
           dict(slice="perc", linear=False, Nk=3, P=4096, M=_M, gamma=1.0, beta_g=1.0, seed=778), _run(0.05, 300, sampler="rrr", thr=0.5, seed=20284), build=_bd, lds=_b)
        for _M, _b, _bd in ((17, 159016, LDS), (18, 168240, GLOBAL))])
_pair(*[_e("le_perclinear_P4096_M%d_pair" % _M, "le", [PERC_P, ("LDS bytes", _b, "le_rrr_lds_bytes + perc_lds_bytes vs kLdsLimit = 163840")],
           dict(slice="perc", linear=True, Nk=3, P=4096, M=_M, gamma=1.0, beta_g=1.0, seed=779), _run(0.03, 300, sampler="rrr", thr=0.5, seed=20285), build=_bd, lds=_b)
        for _M, _b, _bd in ((16, 159024, LDS), (17, 168248, GLOBAL))])

def rejection_free(e):
    """rrrMC proposes from the inner graph's own Boltzmann weights and accepts on the residual alone: over GraphEmpty (the ensembles) or with
    the fields added to GraphEmpty (GraphAddFields) the residual is zero and every move is accepted, by construction.  What such a run
    decides is which site moves; the entries over perceptron slices, GraphAddSubFields and every standardMC entry reject as well."""
    if e.run["sampler"] == "std":
        return False
    return (e.family in ("re", "le") and e.spec["slice"] == "empty") or (e.family == "af" and e.spec["sub"] == 0 and e.spec.get("g") is None)


# GraphQPercStepT under standardMC: Nk M = 4369 * 15 = 65535 in each of the three builds rrrmc_quant_pattern_build names (0 one thread per
# replica, 1 one wavefront with the slices' Stabilities in global memory, 2 with them staged in LDS); and P = 4096 at Nk = 3 on both sides
# of the staging rule (host_quant_pat.hpp:55-59, standardMC: 4 W bytes of spins + 8 + perc_lds_bytes(M, 64)):
#   M = 17 (N = 51): 8 + 8 + 17 * 9216 = 156688 -> 2;   M = 18 (N = 54): 8 + 8 + 18 * 9216 = 165904 -> 1
def quant_std_lds_bytes(Nk, M, PW):
    return _spin_words(Nk * M) * 4 + 8 + M * PW * (2 * 8 + 64 * 2)


ENTRIES += [
    _e("quant_percstep_M15_N65535_%s" % _tag, "quant", [("N", 65535, "Nk M <= 65535 (host_quant_pat.hpp)")],
       dict(Nk=4369, P=64, M=15, Gamma=0.6, beta_g=2.0, seed=800, same_as="quant_percstep_M15_N65535_lds"), _run(1.5, 600, seed=20311), build=_bd, env=_env)
    for _tag, _env, _bd in (("lds", {}, 2), ("wave_no_lds", {"RRRMC_QUANT_NO_LDS": "1"}, 1), ("thread", {"RRRMC_QUANT_NO_WAVE": "1"}, 0))]
_pair(*[_e("quant_percstep_P4096_M%d_pair" % _M, "quant", [PERC_P, ("LDS bytes", _b, "4 W + quant_pat_stage_bytes vs kLdsLimit = 163840")],
           dict(Nk=3, P=4096, M=_M, Gamma=0.6, beta_g=2.0, seed=801), _run(0.3, 300, seed=20312), build=_bd, lds=_b)
        for _M, _b, _bd in ((17, 156688, 2), (18, 165904, 1))])

# GraphQCommQuT under standardMC (Δ2 of the slices in int32 on the quant_pat_kernels.hpp path): Nk M = 21844 * 3 = 65532, the nearest
# admissible value to 65535 (Nk = K1 K2 with both even is a multiple of 4), K1 = 10922, K2 = 2, in the three builds; and P = 4096 at
# K1 = K2 = 2 on both sides of the staging rule, 4 W + 8 + comm_lds_bytes(M, 2, 64, qu) with rows of 2 * 64 * 8 + 4 * 64 * 64 * 2 = 33792 bytes:
#   M = 4 (N = 16): 8 + 8 + 135168 = 135184 -> 2;   M = 5 (N = 20): 8 + 8 + 168960 = 168976 -> 1
def quant_qu_std_lds_bytes(Nk, M, K2, PW):
    return _spin_words(Nk * M) * 4 + 8 + M * (2 * PW * 8 + (K2 + 2) * 64 * PW * 2)


ENTRIES += [
    _e("quant_commqu_M3_N65532_%s" % _tag, "quant", [("N", 65532, "the largest multiple of 4 M <= 65535 at M = 3")],
       dict(qu=True, K1=10922, K2=2, P=64, M=3, Gamma=0.6, beta_g=2.0, seed=806, same_as="quant_commqu_M3_N65532_lds"), _run(1.5, 600, seed=20317), build=_bd, env=_env)
    for _tag, _env, _bd in (("lds", {}, 2), ("wave_no_lds", {"RRRMC_QUANT_NO_LDS": "1"}, 1), ("thread", {"RRRMC_QUANT_NO_WAVE": "1"}, 0))]
_pair(*[_e("quant_commqu_P4096_M%d_pair" % _M, "quant", [("P", 4096, "kCommPmax"), ("LDS bytes", _b, "4 W + quant_pat_stage_bytes vs kLdsLimit = 163840")],
           dict(qu=True, K1=2, K2=2, P=4096, M=_M, Gamma=0.6, beta_g=2.0, seed=807), _run(0.5, 300, seed=20318), build=_bd, lds=_b)
        for _M, _b, _bd in ((4, 135184, 2), (5, 168976, 1))])

# The committee term of the ensembles' rule (host_re.hpp:114): RE over GraphCommStep(3, 3, 4096) slices by M.  A row of Stabilities is
# (2 K2 + 2) PW 8 + (K2 + 1) 64 PW 2 = 4096 + 32768 = 36864 bytes:  M = 4 (N = 36): 2304 + 147456 = 149760;  M = 5 (N = 45): 2336 + 184320 = 186656
def re_comm_lds_bytes(Nk, M, K2, PW):
    return _a8(re_lds_bytes(Nk, M)) + M * ((2 * K2 + 2) * PW * 8 + (K2 + 1) * 64 * PW * 2)


_pair(*[_e("re_commstep_P4096_M%d_pair" % _M, "re", [("P", 4096, "kCommPmax"), ("LDS bytes", _b, "re_rrr_lds_bytes + comm_lds_bytes vs kLdsLimit = 163840")],
           dict(slice="comm", K1=3, K2=3, Nk=9, P=4096, M=_M, gamma=1.0, beta_g=1.0, seed=808), _run(0.05, 300, sampler="rrr", thr=0.5, seed=20319), build=_bd, lds=_b)
        for _M, _b, _bd in ((4, 149760, LDS), (5, 186656, GLOBAL))])

# The sparse Float64 slices' term (host_ens.hpp:137, ens_spf_lds): the LDS build stages the slices' fields, undo records and move_last behind
# the chain's own arrays when both fit, 8 rows (Nk + K + 1) + 4 rows bytes more; crossed by the side L of GraphEARE / GraphEALE(L, 2, M = 3)
# (Nk = L^2, K = 4; the next admissible value is L + 1).  Both sides run the LDS build (rrrmc_ens_build = 1: the chain's own arrays fit);
# what pins the pair is parity on both sides.
#   RE: L = 68 (Nk = 4624): 50152 + 24 * 4629 + 12 = 161260;   L = 69 (Nk = 4761): 51584 + 24 * 4766 + 12 = 165980
#   LE: L = 59 (Nk = 3481): 49184 + 32 * 3486 + 16 = 160752;   L = 60 (Nk = 3600): 50784 + 32 * 3605 + 16 = 166160
def spf_lds_bytes(ens, L, M, K=4):
    rows, base = (M, re_lds_bytes(L * L, M)) if ens == "re" else (M + 1, le_lds_bytes(L * L, M))
    return _a8(base) + 8 * rows * (L * L + K + 1) + 4 * rows


SPF_PAIRS = []
for _ens, _shapes in (("re", ((68, 161260), (69, 165980))), ("le", ((59, 160752), (60, 166160)))):
    _two = [_e("%s_ea_L%d_M3_pair" % (_ens, _L), _ens, [("slice-state LDS bytes", _b, "ens_spf_lds vs kLdsLimit = 163840")],
               dict(slice="spf", L=_L, Nk=_L * _L, M=3, gamma=1.2, beta_g=1.5, seed=810), _run(0.6, 600, sampler="rrr", thr=0.5, seed=20321), build=LDS)
            for _L, _b in _shapes]
    ENTRIES.extend(_two)
    SPF_PAIRS.append((_two[0].name, _two[1].name))

# GraphPercXEntr's table in LDS or in global memory (host_xentr.hpp:113-123), crossed by N (odd: the next admissible value is N + 2), P = 65.
# rrrmc_xentr_build names the wave / thread build only, so what pins these pairs is parity on both sides; the bytes are written for the record.
#   thread build (RRRMC_XENTR_NO_WAVE=1), (N + 1) 8:            N = 20479: 163840 (the limit itself);  N = 20481: 163856
#   wave build, 2 * 64 * 8 + (N + 1) 8 + 2 * 64 * 2 + 4 W:      N = 20005: 1024 + 160048 + 256 + 2504 = 163832;  N = 20007: 163848
XENTR_PAIRS = []
for _tag, _env, _bd, _shapes in (("thread", {"RRRMC_XENTR_NO_WAVE": "1"}, 1, ((20479, 163840), (20481, 163856))), ("wave", {}, 2, ((20005, 163832), (20007, 163848)))):
    _two = [_e("xentr_%s_N%d_P65_pair" % (_tag, _N), "xentr", [("table LDS bytes", _b, "xentr_lds_bytes / (N + 1) 8 vs kLdsLimit = 163840")],
               dict(N=_N, P=65, lam=1.0, seed=809), _run(1.0, 300, seed=20320), build=_bd, env=_env) for _N, _b in _shapes]
    ENTRIES.extend(_two)
    XENTR_PAIRS.append((_two[0].name, _two[1].name))

BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES)
NAMES = [e.name for e in ENTRIES]


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def crafted_patterns(N, counts, seed):
    """(c, ξ): a seeded configuration c and P x N patterns — counts[0] equal to c, counts[1] its complement, counts[2] at Δ = +1 (c with
    (N - 1) / 2 seeded bits flipped), interleaved so that every mask word holds both ends"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, N, dtype=np.uint8)
    rows = [c] * counts[0] + [1 - c] * counts[1]
    for _ in range(counts[2]):
        x = c.copy()
        x[rng.choice(N, (N - 1) // 2, replace=False)] ^= 1
        rows.append(x)
    order = rng.permutation(len(rows))
    xi = np.stack([rows[k] for k in order])
    c.setflags(write=False)
    xi.setflags(write=False)
    return c, xi


def degree_instance(seed):
    """N = 9 and 65535 clauses of 8 literals (of the 9 variables each leaves one of 1 .. 8 out), all holding variable 0, seeded literal bits"""
    rng = np.random.default_rng(seed)
    out = rng.integers(1, 9, 65535)
    A = [[i for i in range(9) if i != o] for o in out.tolist()]
    J = rng.integers(0, 2, (65535, 8)).tolist()
    return 9, A, J


class SatVec:
    """GraphSAT, numpy-vectorised: S[a] = the number of true literals of clause a, kept under flips; ΔE of variable i read from the clauses
    T[i] alone (those i alone satisfies minus the unsatisfied ones).  Built from a product GraphSAT's padded clause arrays; it has the
    interfaces of sat_reference.ClauseCache (energy, delta_energy, update_cache) and of a slice (delta, flip_update).
    tests/test_limit_instances_cpu.py pins it to the plain ClauseCache at small shapes: energies, ΔE at every site, trajectories."""

    def __init__(self, X):
        self.N = X.N
        self.vars, self.mask = np.asarray(X._vars, np.int64), np.asarray(X._vars) >= 0
        self.lits = np.asarray(X._lits, np.int64)
        cl, k = np.nonzero(self.mask)                                    # clause order
        v = self.vars[cl, k]
        order = np.argsort(v, kind="stable")
        self.tc, self.tl = cl[order], self.lits[cl, k][order]            # T[i] and the literal bit of i there, CSR by variable
        self.ptr = np.searchsorted(v[order], np.arange(self.N + 1))
        self.S, self.s = None, None

    def energy(self, s):
        self.s = s
        self.S = ((self.lits == np.asarray(s, np.int64)[np.where(self.mask, self.vars, 0)]) & self.mask).sum(axis=1)
        return int((self.S == 0).sum())

    def delta(self, s, i):
        a = slice(self.ptr[i], self.ptr[i + 1])
        Sa = self.S[self.tc[a]]
        return int(((Sa == 1) & (self.tl[a] == int(s[i]))).sum() - (Sa == 0).sum())

    def flip_update(self, s, i):                                         # after the flip of s[i]
        a = slice(self.ptr[i], self.ptr[i + 1])
        self.S[self.tc[a]] += np.where(self.tl[a] == int(s[i]), 1, -1)

    def delta_energy(self, i):
        return self.delta(self.s, i)

    def update_cache(self, i):
        self.flip_update(self.s, i)


@functools.lru_cache(maxsize=1)
def crafted_qu(K1, P, seed):
    """(c, ξ, y) for GraphCommQu(K1, 2): patterns 0 and 1 equal c on unit 0 and differ from it in K1 / 2 seeded places of unit 1
    (Δ1 = (K1, 0)), labels 1 and 0: Δ2 = +K1^2 and -K1^2; the other patterns, labels and c are seeded draws"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, 2 * K1, dtype=np.uint8)
    xi = rng.integers(0, 2, (P, 2 * K1), dtype=np.uint8)
    y = rng.integers(0, 2, P, dtype=np.uint8)
    row = c.copy()
    row[K1 + rng.choice(K1, K1 // 2, replace=False)] ^= 1
    xi[0], xi[1], y[0], y[1] = row, row, 1, 0
    return c, xi, y


class CommQuVec:
    """GraphCommQu, numpy-vectorised: Δ1[K2, P] and Δ2[P] kept under flips; ΔE over all patterns as
    comm_qu_reference.delta_from_stabilities counts it, [Δ2 after the move <= 0] - [Δ2 <= 0].  Pinned to the plain CommQuRef at small shapes."""

    def __init__(self, K2, xi, y):
        self.xi = np.asarray(xi, np.int64)
        self.P, self.N = self.xi.shape
        self.K2, self.K1 = K2, self.N // K2
        self.co = np.where(2 * (np.arange(K2) + 1) <= K2, 1, -1)[:, None] * (2 * np.asarray(y, np.int64) - 1)[None, :]

    def energy(self, s):
        mism = (self.xi ^ np.asarray(s, np.int64)[None, :]).reshape(self.P, self.K2, self.K1).sum(axis=2)
        self.d1 = (self.K1 - 2 * mism).T.copy()
        self.d2 = (self.co * self.d1 ** 2).sum(axis=0)
        return int((self.d2 <= 0).sum())

    def delta(self, s, move):
        k = move // self.K1
        x = self.xi[:, move] ^ int(s[move])
        moved = self.d2 + self.co[k] * 4 * (1 - (1 - 2 * x) * self.d1[k])
        return int((moved <= 0).sum() - (self.d2 <= 0).sum())

    def flip_update(self, s, move):                                      # after the flip of s[move]
        k = move // self.K1
        old = self.d1[k]
        new = old + (2 - 4 * (self.xi[:, move] ^ int(s[move])))
        self.d2 = self.d2 + self.co[k] * (new ** 2 - old ** 2)
        self.d1[k] = new

    def members(self):
        """the misclassified patterns {Δ2 <= 0}: the boundary the energy counts"""
        return (frozenset(np.nonzero(self.d2 <= 0)[0].tolist()),)


class SliceSKLean(RE.SliceSK):
    """re_reference.SliceSK with one coupling matrix shared by all slices (int8, handed in) and energy() as one matrix operation; delta and
    flip_update are the plain class's own.  Pinned to SliceSK at small shapes by tests/test_limit_instances_cpu.py."""

    def __init__(self, J8, Nk):
        self.Nk, self.sN, self.J = Nk, np.sqrt(Nk), J8
        self.lf = np.zeros(Nk, np.int64)
        self.lfl = np.zeros(Nk, np.int64)
        self.move_last = -1

    def energy(self, s):
        N = self.Nk
        s = np.asarray(s, np.int64)
        sc = (self.J ^ s[None, :].astype(np.int8)).sum(axis=1, dtype=np.int64)
        lf = -(2 * s - 1) * (N - 1 - 2 * sc)
        self.lf = 2 * (-lf + 2 * s)
        n = -2 * int(s.sum()) + int(lf.sum())
        assert n % 2 == 0
        self.move_last = -1
        self.lfl = np.zeros(N, np.int64)
        return (n // 2) / float(self.sN)


def sk_bits(Jc, Nk):
    """[Nk, chunks] coupling rows -> Nk x Nk int8 of 0/1"""
    return np.unpackbits(np.ascontiguousarray(Jc, "<u8").view(np.uint8), axis=1, bitorder="little")[:, :Nk].astype(np.int8)


class CommVec:
    """GraphCommStep / GraphCommReLU, numpy-vectorised: Δ1[K2, P] and Δ2[P] kept under flips, the p / m sets read as functions of them
    (comm_reference.masks_of) and ΔE as comm_reference.delta_from_masks counts it.  tests/test_limit_instances_cpu.py pins it to the plain
    CommStepRef / CommReLURef at small shapes: energies, ΔE at every site, trajectories."""

    def __init__(self, K2, xi, y=None):
        self.xi = np.asarray(xi, np.int64)
        self.P, self.N = self.xi.shape
        self.K2, self.K1, self.relu = K2, self.N // K2, y is not None
        self.c = np.where(2 * (np.arange(K2) + 1) <= K2, 1, -1)
        self.o = None if y is None else 2 * np.asarray(y, np.int64) - 1

    def _d2(self):
        if self.relu:
            return self.o * (self.c[:, None] * np.maximum(self.d1, 0)).sum(axis=0)
        return np.sign(self.d1).sum(axis=0)

    def energy(self, s):
        mism = (self.xi ^ np.asarray(s, np.int64)[None, :]).reshape(self.P, self.K2, self.K1).sum(axis=2)
        self.d1 = (self.K1 - 2 * mism).T.copy()
        self.d2 = self._d2()
        return int((self.d2 <= 0).sum() if self.relu else (self.d2 < 0).sum())

    def delta(self, s, move):
        k = move // self.K1
        col = (self.xi[:, move] ^ int(s[move])).astype(bool)
        d1, d2 = self.d1[k], self.d2
        if not self.relu:
            return int(((d2 == 1) & (d1 == 1) & ~col).sum() - ((d2 == -1) & (d1 == -1) & col).sum())
        A, AZ, eq, p2, m2 = d1 > 0, d1 >= 0, self.o == self.c[k], d2 == 2, d2 == 0
        return int((p2 & eq & A & ~col).sum() + (p2 & ~eq & AZ & col).sum() - (m2 & eq & AZ & col).sum() - (m2 & ~eq & A & ~col).sum())

    def flip_update(self, s, move):                                      # after the flip of s[move]
        k = move // self.K1
        old = self.d1[k]
        new = old + (2 - 4 * (self.xi[:, move] ^ int(s[move])))
        if self.relu:
            self.d2 = self.d2 + self.o * self.c[k] * (np.maximum(new, 0) - np.maximum(old, 0))
        else:
            self.d2 = self.d2 + np.sign(new) - np.sign(old)
        self.d1[k] = new

    def members(self):
        """(p2, m2) as comm_reference.masks_of reads them from Δ2: {Δ2 = 1}, {Δ2 = -1} (step) or {Δ2 = 2}, {Δ2 = 0} (ReLU)"""
        a, b = (2, 0) if self.relu else (1, -1)
        return frozenset(np.nonzero(self.d2 == a)[0].tolist()), frozenset(np.nonzero(self.d2 == b)[0].tolist())


def fields(N, seed=5):
    """the fields of tests/test_gpu_add_fields_parity.py: Gaussian, with exact zeros of both signs and two fields of ±10"""
    h = np.random.default_rng(seed).normal(size=N)
    h[0] = 0.0
    h[N // 2] = -0.0
    h[1], h[N - 2] = 10.0, -10.0
    return h


@functools.lru_cache(maxsize=2)
def graph(pkg, name):
    """the product graph of an entry (built on the host: no device is touched)"""
    e = BY_NAME[name]
    sp = e.spec
    if e.family == "perc":
        G = pkg.GraphPercLinear if sp["linear"] else pkg.GraphPercStep
        if "crafted" in sp:
            return G.from_patterns(crafted_patterns(sp["N"], sp["crafted"], sp["seed"])[1])
        return G(sp["N"], sp["P"], seed=sp["seed"])
    if e.family == "xentr":
        return pkg.GraphPercXEntr(sp["N"], sp["P"], sp["lam"], seed=sp["seed"])
    if e.family == "quant" and sp.get("qu"):
        return pkg.GraphQCommQuT(sp["K1"], sp["K2"], sp["P"], sp["M"], sp["Gamma"], sp["beta_g"], seed=sp["seed"])
    if e.family == "quant":
        return pkg.GraphQPercStepT(sp["Nk"], sp["P"], sp["M"], sp["Gamma"], sp["beta_g"], seed=sp["seed"])
    if e.family == "comm":
        if sp.get("crafted_qu"):
            _, xi, y = crafted_qu(sp["K1"], sp["P"], sp["seed"])
            return pkg.GraphCommQu.from_patterns(2, xi, y)
        G = pkg.GraphCommQu if sp.get("qu") else pkg.GraphCommReLU if sp["relu"] else pkg.GraphCommStep
        return G(sp["K1"], sp["K2"], sp["P"], seed=sp["seed"])
    if e.family == "sat":
        if sp["kind"] == "degree":
            return pkg.GraphSAT.from_clauses(*degree_instance(sp["seed"]))
        return pkg.GraphSAT(sp["N"], sp["K"], sp["alpha"], seed=sp["seed"])
    if e.family in ("re", "le") and sp["slice"] == "spf":
        return (pkg.GraphEARE if e.family == "re" else pkg.GraphEALE)(sp["L"], 2, sp["M"], sp["gamma"], sp["beta_g"], seed=sp["seed"])
    if e.family in ("re", "le"):
        X1 = None
        if sp["slice"] == "sat":
            X1 = pkg.GraphSAT(sp["Nk"], sp["K"], sp["alpha"], seed=sp["seed"])
        if sp["slice"] == "sk":
            X1 = pkg.GraphSK(sp["Nk"], seed=sp["seed"])
        if sp["slice"] == "comm":
            X1 = pkg.GraphCommStep(sp["K1"], sp["K2"], sp["P"], seed=sp["seed"])
        if sp["slice"] == "perc":
            X1 = (pkg.GraphPercLinear if sp["linear"] else pkg.GraphPercStep)(sp["Nk"], sp["P"], seed=sp["seed"])
        G = pkg.GraphRobustEnsemble if e.family == "re" else pkg.GraphLocalEntropy
        return G(sp["Nk"], sp["M"], sp["gamma"], sp["beta_g"], X1)
    if e.family == "af":
        g = None
        if sp.get("g") == "sat":
            g = pkg.GraphSAT(sp["N"], sp["K"], sp["alpha"], seed=sp["seed"])
        elif sp.get("g") == "perc":
            g = pkg.GraphPercStep(sp["N"], sp["P"], seed=sp["seed"])
        return (pkg.GraphAddSubFields if sp["sub"] else pkg.GraphAddFields)(fields(sp["N"]), g)
    raise KeyError(e.family)


def pack(bits):
    """[R, N] 0/1 -> [R, ceil(N / 64)] chunks"""
    bits = np.atleast_2d(bits)
    pad = np.zeros((bits.shape[0], 64 * ((bits.shape[1] + 63) // 64)), np.uint8)
    pad[:, :bits.shape[1]] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u8")


def unpack(chunks, N):
    """one row of chunks -> N 0/1 as int64 (what the references take)"""
    return np.unpackbits(np.ascontiguousarray(chunks, "<u8").view(np.uint8), bitorder="little")[:N].astype(np.int64)


def start_configs(pkg, oracle, name):
    """[R, chunks]: the configurations the chains start from — the INIT stream of the run's seed (what Engine.init_spins_random gives), or,
    for the entries with a ``start``, one numpy-built configuration for every chain"""
    e = BY_NAME[name]
    sp, R = e.spec, e.run["R"]
    N = graph(pkg, name).N
    kind = sp.get("start")
    if kind is None:
        return oracle.init_configs(e.run["seed"], 0, R, N)
    if kind == "crafted_qu":
        c = crafted_qu(sp["K1"], sp["P"], sp["seed"])[0]
    elif kind == "crafted":
        c = crafted_patterns(sp["N"], sp["crafted"], sp["seed"])[0]
    else:                                    # "margin": pattern 0 with (N - 1) / 2 bits flipped, Δ_0 = +1
        c = graph(pkg, name).patterns()[0].copy()
        c[:(N - 1) // 2] ^= 1
    return np.repeat(pack(c), R, axis=0)


# ---- the reference runs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _patterns(X):
    return np.unpackbits(np.ascontiguousarray(X.xi, "<u8").view(np.uint8), axis=1, bitorder="little")[:, :X.N].astype(np.int64)


@functools.lru_cache(maxsize=1)
def _sk_matrix(X1):
    return sk_bits(X1.J, X1.N)


def _slices(e, X):
    """the int64 P x N pattern matrix the perceptron / committee references share (unpacked once per graph; the last one is kept); for SK
    slices the shared int8 coupling matrix"""
    if e.spec.get("slice") == "sk":
        return _sk_matrix(X.X1)
    return _patterns(X.X1 if e.family in ("re", "le", "af", "quant") else X)


def _reference_of(e, X, xi):
    sp = e.spec
    if e.family == "perc":
        return PR.make(xi, sp["linear"])
    if e.family == "xentr":
        return XR.PercXEntrRef(xi, Hs=X.Hs)
    if e.family == "quant" and sp.get("qu"):
        return QP.GraphQuantRef(X.Nk, X.M, X.fourK, [CommQuVec(X.X1.K2, xi, X.X1.labels()) for _ in range(X.M)])
    if e.family == "quant":
        return QP.make_reference(X)
    if e.family == "sat":
        return SatVec(X)
    if e.family == "comm":
        return CommQuVec(X.K2, xi, X.labels()) if sp.get("qu") else CommVec(X.K2, xi, X.labels())
    if e.family == "af":
        if sp.get("g") == "sat":
            return AF.AddFields(X.fields, SatVec(X.X1), sp["sub"])
        if sp.get("g") == "perc":
            return AF.AddFields(X.fields, PR.make(xi, False), sp["sub"])
        return AF.reference_of(X)
    Ref = RE if e.family == "re" else LE
    if sp["slice"] == "spf":
        return (SP.make_re if e.family == "re" else SP.make_le)(X.X1.A, X.X1.J, sp["M"], sp["gamma"], sp["beta_g"])
    if sp["slice"] in ("sk", "comm"):
        rows = sp["M"] + (e.family == "le")
        Xe = Ref.make_ensemble(sp["Nk"], sp["M"], sp["gamma"], sp["beta_g"], "empty")
        sl = [SliceSKLean(xi, sp["Nk"]) if sp["slice"] == "sk" else CommVec(X.X1.K2, xi, None) for _ in range(rows)]
        Xe.X1 = sl[:sp["M"]]
        if e.family == "le":
            Xe.Xc = sl[-1]
        return Xe
    if sp["slice"] == "sat":
        Xe = Ref.make_ensemble(sp["Nk"], sp["M"], sp["gamma"], sp["beta_g"], "empty")
        Xe.X1 = [SatVec(X.X1) for _ in range(sp["M"])]
        if e.family == "le":
            Xe.Xc = SatVec(X.X1)
        return Xe
    if sp["slice"] == "perc":
        return (PR.re_ensemble if e.family == "re" else PR.le_ensemble)(xi, sp["linear"], sp["M"], sp["gamma"], sp["beta_g"])
    return Ref.make_ensemble(sp["Nk"], sp["M"], sp["gamma"], sp["beta_g"], "empty")


def perc_deltas(xi, s):
    """Δ_a = σ·ξ_a of every pattern, in exact integers"""
    return xi.shape[1] - 2 * (xi ^ np.asarray(s, np.int64)[None, :]).sum(axis=1)


def perc_energy_definition(xi, linear, s):
    """the energy from the definition, in Python integers (linear: the numerator n of 2 n / sqrt(N))"""
    d = [int(x) for x in perc_deltas(xi, s)]
    return sum((-x - 1) // 2 + 1 for x in d if x < 0) if linear else sum(x < 0 for x in d)


@functools.lru_cache(maxsize=None)
def reference(pkg, oracle, name):
    """The reference result of an entry, computed once and shared (read it, do not change it): per replica r a dict with
    ``E0``; ``Es`` / ``acc`` / ``staged`` / ``s`` (final configuration) / ``E`` (tracked energy) / ``cache`` for each of the two calls;
    ``members`` = the perceptron's (p, m) sets at the start and after each call; ``obs`` = the ensembles' observables at the end."""
    e = BY_NAME[name]
    rn, sp = e.run, e.spec
    if sp.get("same_as", name) != name:
        assert BY_NAME[sp["same_as"]].spec == sp and BY_NAME[sp["same_as"]].run == rn
        return reference(pkg, oracle, sp["same_as"])
    X = graph(pkg, name)
    N = X.N
    xi = _slices(e, X) if (e.family in ("perc", "xentr", "comm") or sp.get("slice") in ("perc", "sk", "comm") or sp.get("g") == "perc"
                           or (e.family == "quant" and sp.get("qu"))) else None
    C0 = start_configs(pkg, oracle, name)
    out = []
    for r in range(rn["R"]):
        s = unpack(C0[r], N)
        res = dict(calls=[])
        for c in range(2):
            Xr = _reference_of(e, X, xi)
            if rn["sampler"] == "std":
                if e.family == "quant":
                    E0 = Xr.energy(s)
                    es, E, acc = QP.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                    res["obs"] = dict(renergies=[float(x) for x in Xr.renergies()])
                elif e.family == "comm":
                    E0 = Xr.energy(s)
                    if c == 0:
                        res["members"] = [Xr.members()]
                    es, E, acc = CR.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                    res["members"].append(Xr.members())
                elif e.family == "sat":
                    E0 = Xr.energy(s)
                    es, E, acc = SR.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                elif e.family == "xentr":
                    E0 = Xr.energy(s)
                    es, E, acc = XR.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                    res.setdefault("step_energy", []).append(Xr.step_energy())
                elif e.family == "perc":
                    E0 = Xr.energy(s)
                    members = [Xr.members()] if c == 0 else res["members"]
                    es, E, acc = PR.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                    members.append(Xr.members())
                    res["members"] = members
                else:
                    E0 = Xr.energy(s)          # (a fresh call starts from energy(X, C): the samplers are handed what they would compute)
                    Ref = RE if e.family == "re" else LE
                    es, E, acc = Ref.standard_mc(Xr, s, rn["beta"], rn["iters"], rn["step"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], E=E0)
                call = dict(Es=es, acc=acc, staged=None, E=E, cache=None)
            else:
                Run = AF.AfRun if e.family == "af" else (RE if e.family == "re" else LE).RrrRun
                run = Run(Xr, s, rn["beta"], rn["seed"], oracle, replica=r, it0=c * rn["iters"], staged_thr=rn["thr"])
                E0 = run.E
                es = run.run(rn["iters"], rn["step"])
                call = dict(Es=es, acc=run.accepted, staged=run.staged_its, E=run.E, cache=run.cache_view())
            if c == 0:
                res["E0"] = E0
            call["s"] = s.copy()
            res["calls"].append(call)
        if e.family in ("re", "le"):
            res["obs"] = observables(e, xi, s, X)
        out.append(res)
    return out


def observables(e, xi, s, X=None):
    """REenergies, or (LEenergies, cenergy, distances), of configuration s from the definition"""
    sp = e.spec
    rows = sp["M"] + (e.family == "le")
    if sp["slice"] == "spf":
        A, J, M = X.X1.A, X.X1.J, sp["M"]
        if e.family == "re":
            return dict(re=SP.re_energies(A, J, M, s))
        return dict(le=SP.le_energies(A, J, M, s), c=SP.cenergy(A, J, M, s), d=LE.distances(sp["Nk"], M, s))
    if sp["slice"] == "perc":
        es = [float(PR.make(xi, sp["linear"]).energy(np.asarray(s[k::rows], np.int64))) for k in range(rows)]
    elif sp["slice"] == "sk":
        es = [float(SliceSKLean(xi, sp["Nk"]).energy(s[k::rows])) for k in range(rows)]
    elif sp["slice"] == "comm":
        es = [float(CommVec(X.X1.K2, xi, None).energy(s[k::rows])) for k in range(rows)]
    elif sp["slice"] == "sat":
        es = [float(SR.pure_energy(X.X1.A, X.X1.J, s[k::rows])) for k in range(rows)]
    else:
        es = [0.0] * rows
    if e.family == "re":
        return dict(re=es)
    return dict(le=es[1:], c=es[0], d=LE.distances(sp["Nk"], sp["M"], s))
