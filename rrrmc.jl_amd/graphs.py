"""Graph and configuration objects: the data the drop-in boundary marshals.

Indices are 0-based here; the Julia glue converts from the reference's 1-based tuples.
"""
import ctypes as C
import math

import numpy as np

from ._lib import check, lib

DEFAULT_SEED = 167432777111  # src/RRRMC.jl:82


def nchunks(N):
    return (int(N) + 63) // 64


class Config:
    """R configurations of N spins in Julia BitVector chunk layout (src/Interface.jl:21-29).

    ``s[r, c]`` is chunk c of replica r; spin x of replica r is bit (x & 63) of ``s[r, x >> 6]``,
    sigma = 2*bit - 1.  ``Config(N, R)`` alone is all-zeros; random initialisation is done on the
    device by ``Engine.init_spins_random`` (the reference draws rand!(BitVector), Interface.jl:26).
    """

    def __init__(self, N, R=1, s=None):
        self.N = int(N)
        self.R = int(R)
        if s is None:
            s = np.zeros((self.R, nchunks(N)), np.uint64)
        s = np.ascontiguousarray(s, np.uint64).reshape(self.R, nchunks(N))
        self.s = s

    def __len__(self):
        return self.N

    def copy(self):
        return Config(self.N, self.R, self.s.copy())

    def __eq__(self, other):
        return isinstance(other, Config) and self.N == other.N and self.R == other.R and bool((self.s == other.s).all())

    def bits(self):
        """[R, N] array of 0/1."""
        x = np.arange(self.N)
        return ((self.s[:, x >> 6] >> (x & 63).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)

    @staticmethod
    def from_bits(bits):
        bits = np.atleast_2d(np.asarray(bits))
        R, N = bits.shape
        pad = np.zeros((R, 64 * nchunks(N)), np.uint8)          # bit x of a row is bit (x & 63) of chunk x >> 6: little-endian bit order
        pad[:, :N] = bits
        return Config(N, R, np.packbits(pad, axis=1, bitorder="little").view("<u8"))


def level_units(LEV):
    """LEV as given to the reference's constructors -> (units, mul, div): value = units * mul / div.
    Int levels: (LEV, 1, 1.0).  Float64 levels become DFloat64 (RRG.jl:162,324; EA.jl:193,357): the Int64 t = round(x * 10^5)
    (src/DFloats.jl:23, ties to even); units = t / g with g = gcd of the |t|, (mul, div) = (g, 1e5).  Rational levels
    (fractions.Fraction; runtests.jl:40) over the common denominator d: units = numerators / g, (mul, div) = (g, d)."""
    from fractions import Fraction
    LEV = tuple(LEV)
    if all(isinstance(l, (int, np.integer)) for l in LEV):
        return tuple(int(l) for l in LEV), 1, 1.0
    if all(isinstance(l, (int, np.integer, Fraction)) for l in LEV):
        d = 1
        for l in LEV:
            d = d * Fraction(l).denominator // math.gcd(d, Fraction(l).denominator)
        t = [int(Fraction(l) * d) for l in LEV]
        div = float(d)
    else:
        t = [int(np.rint(float(l) * 100000.0)) for l in LEV]
        div = 100000.0
    g = 0
    for x in t:
        g = math.gcd(g, abs(x))
    g = max(g, 1)
    return tuple(x // g for x in t), g, div


class _DeviceGraph:
    """What ``Engine`` asks of a graph to put it on the device: ``_create`` makes the single-device context, ``_multi_args`` names it to
    ``rrrmc_ctx_create_multi``, ``_upload`` makes the ``rrrmc_set_*`` calls (``_upload_couplings`` alone when the graph is the slice graph
    of a GraphQuant or of an ensemble), and five facts.  The defaults are those of most families; a class overrides what differs."""
    _f64 = True             # the device's energy word is Float64 (also behind the Int energies of the perceptrons and committee machines), else Int64
    _units = False          # device energies are int64 level units: energy_value converts
    _fields_f64 = False     # the cached local fields are Float64 (GraphSK's are integer: SK.jl:33)
    _rrr_classes = 16       # ΔE classes in Engine.rrr_cache
    _staged_thr = 0.5       # rrrMC's default: RRRMC.jl:162-164 (SimpleGraph 0.8, DiscrGraph 0.5) and :226 (DoubleGraph 0.5)

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create(ctx, self.model_kind, self.N, self.K, R, device, replica0))

    def _multi_args(self):
        """(kind, N, K, M) of rrrmc_ctx_create_multi"""
        return self.model_kind, self.N, self.K, 0

    def _create_multi(self, ctx, R, ids, replica0):
        """the same context over the devices ``ids``"""
        kind, N, K, M = self._multi_args()
        check(lib().rrrmc_ctx_create_multi(ctx, kind, N, K, M, R, ids, len(ids), replica0))

    def _upload(self, ctx):
        self._upload_couplings(ctx)


class _SparseLevelsGraph:
    """GraphRRG{ET,LEV,K} / GraphEA{ET,LEV,2D} with levels other than (-1, 1) (RRG.jl:116-162, EA.jl:138-193): couplings in level
    units, energies come back from the device in units and are returned as ``units * lev_mul / lev_div`` (exact integers for Int
    levels, the Float64 value of the reference's DFloat64 / Rational otherwise)."""
    model_kind = 7          # RRRMC_MODEL_SPARSE_LEVELS
    _f64, _units = False, True

    def _upload(self, ctx):
        check(lib().rrrmc_set_graph_levels(ctx, self.A, self.J, np.asarray(self.LEV, np.int32), len(self.LEV), self.ea_form), ctx)
        check(lib().rrrmc_set_level_scale(ctx, self.lev_mul, self.lev_div), ctx)

    def _init_levels(self, A, J, LEV, ea_form):
        self.levels = tuple(LEV)
        self.LEV, self.lev_mul, self.lev_div = level_units(LEV)
        if len(set(self.LEV)) != len(self.LEV):
            raise ValueError("repeated levels in LEV: %r" % (LEV,))                   # RRG.jl:100
        if max(abs(u) for u in self.LEV) > 127:
            raise NotImplementedError("levels %r need more than 8 bits per coupling after reduction by their gcd" % (LEV,))
        A = np.ascontiguousarray(A, np.int32)
        self.N, self.K = A.shape
        self.A = A
        if J is None:
            J = np.zeros(A.shape, np.int8)
            check(lib().rrrmc_gen_couplings_lev(self.N, self.K, A, self._seed, np.asarray(self.LEV, np.int32), len(self.LEV), J))
        J = np.ascontiguousarray(J, np.int8)
        if J.shape != A.shape:
            raise ValueError("incompatible shapes of A and J: %r, %r" % (A.shape, J.shape))
        if not np.isin(J, self.LEV).all():
            raise ValueError("the given J is incompatible with levels %r" % (LEV,))  # RRG.jl:130
        self.J = J
        self.ea_form = ea_form
        self.energy_dtype = np.int64 if self.lev_div == 1.0 else np.float64

    def energy_value(self, units):
        """Level units -> the energy in the caller's terms (Int, or Float64(::DFloat64) = t / 10^5)."""
        u = np.asarray(units, np.int64) * self.lev_mul
        return u if self.lev_div == 1.0 else u / self.lev_div


class _SparsePM1Graph(_DeviceGraph):
    """Common part of GraphRRG / GraphEA with LEV = (-1, 1): neighbour table A[N, K], couplings J[N, K]."""
    model_kind = 1          # RRRMC_MODEL_SPARSE_PM1
    energy_dtype = np.int64
    _f64 = False

    def _upload(self, ctx):
        check(lib().rrrmc_set_graph(ctx, self.A, self.J), ctx)

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_quant_slice_form(ctx, 1 if isinstance(self, GraphEA) else 0), ctx)
        check(lib().rrrmc_set_graph(ctx, self.A, self.J), ctx)

    def __init__(self, A, J):
        A = np.ascontiguousarray(A, np.int32)
        J = np.ascontiguousarray(J, np.int8)
        if A.ndim != 2 or A.shape != J.shape:
            raise ValueError("incompatible shapes of A and J: %r, %r" % (A.shape, J.shape))
        if not np.isin(J, (-1, 1)).all():
            raise ValueError("the given J is incompatible with levels (-1, 1)")   # RRG.jl:130
        self.N, self.K = A.shape
        self.A, self.J = A, J


class GraphRRG(_SparsePM1Graph):
    """``GraphRRG(N, K)`` — random regular graph, +-1 couplings (src/graphs/RRG.jl:140-162).

    ``GraphRRG.from_AJ(A, J)`` is the inner constructor ``GraphRRG{Int,(-1,1),K}(A, J)`` (RRG.jl:122).
    The disorder comes from the GRAPH / COUPLING Philox streams of ``seed`` (the reference uses the
    global RNG, RRG.jl:45,155).
    """

    def __new__(cls, N=None, K=None, LEV=(-1, 1), seed=DEFAULT_SEED):
        if cls is GraphRRG and (not _is_pm1(LEV) or (K is not None and int(K) > PM1_MAX_K)):
            return object.__new__(GraphRRGLevels)        # GraphRRG{ET,LEV,K} with general levels: its own device context
        return object.__new__(cls)

    def __init__(self, N, K, LEV=(-1, 1), seed=DEFAULT_SEED):
        A = np.zeros((int(N), int(K)), np.int32)
        check(lib().rrrmc_gen_rrg(N, K, seed, A))
        J = np.zeros((int(N), int(K)), np.int8)
        check(lib().rrrmc_gen_couplings_pm1(N, K, A, seed, J))
        super().__init__(A, J)

    @classmethod
    def from_AJ(cls, A, J, LEV=(-1, 1)):
        """``GraphRRG{ET,LEV,K}(A, J)`` (RRG.jl:122); J in level units when LEV is not (-1, 1)."""
        if not _is_pm1(LEV) or np.shape(A)[1] > PM1_MAX_K:
            self = object.__new__(GraphRRGLevels)
            self._init_levels(A, J, LEV, 0)
            return self
        self = object.__new__(cls)
        _SparsePM1Graph.__init__(self, A, J)
        return self


# the bit-sliced +-J kernels count unsatisfied bonds in 3 bit planes (K <= 7); beyond that a +-J graph is a general-level graph with
# LEV = (-1, 1): same couplings (same COUPLING draws), same chains, integer energies, one thread per replica
PM1_MAX_K = 7


def _is_pm1(LEV):
    LEV = tuple(LEV)
    return LEV == (-1, 1) and all(isinstance(l, (int, np.integer)) for l in LEV)


class GraphRRGLevels(_SparseLevelsGraph, GraphRRG):
    """``GraphRRG(N, K, LEV)`` with LEV other than (-1, 1): Int, Float64 (-> DFloat64) or Fraction levels (test/runtests.jl:37-40)."""

    def __init__(self, N, K, LEV=(-1, 1), seed=DEFAULT_SEED):
        A = np.zeros((int(N), int(K)), np.int32)
        check(lib().rrrmc_gen_rrg(N, K, seed, A))
        self._seed = seed
        self._init_levels(A, None, LEV, 0)


class GraphEA(_SparsePM1Graph):
    """``GraphEA(L, D)`` — Edwards-Anderson lattice, +-1 couplings (src/graphs/EA.jl:171-193)."""

    def __new__(cls, L=None, D=None, LEV=(-1, 1), seed=DEFAULT_SEED):
        if cls is GraphEA and (not _is_pm1(LEV) or (D is not None and 2 * int(D) > PM1_MAX_K)):
            return object.__new__(GraphEALevels)
        return object.__new__(cls)

    def __init__(self, L, D, LEV=(-1, 1), seed=DEFAULT_SEED):
        N = int(L) ** int(D)
        A = np.zeros((N, 2 * int(D)), np.int32)
        check(lib().rrrmc_gen_ea(L, D, A))
        J = np.zeros((N, 2 * int(D)), np.int8)
        check(lib().rrrmc_gen_couplings_pm1(N, 2 * int(D), A, seed, J))
        super().__init__(A, J)
        self.L, self.D = int(L), int(D)

    @classmethod
    def from_AJ(cls, A, J, LEV=(-1, 1)):
        if not _is_pm1(LEV) or np.shape(A)[1] > PM1_MAX_K:
            self = object.__new__(GraphEALevels)
            self._init_levels(A, J, LEV, 1)
            return self
        self = object.__new__(cls)
        _SparsePM1Graph.__init__(self, A, J)
        return self


class GraphEALevels(_SparseLevelsGraph, GraphEA):
    """``GraphEA(L, D, LEV)`` with LEV other than (-1, 1) (test/runtests.jl:47-50, 57-60)."""

    def __init__(self, L, D, LEV=(-1, 1), seed=DEFAULT_SEED):
        N = int(L) ** int(D)
        A = np.zeros((N, 2 * int(D)), np.int32)
        check(lib().rrrmc_gen_ea(L, D, A))
        self._seed = seed
        self._init_levels(A, None, LEV, 1)
        self.L, self.D = int(L), int(D)


class _SparseF64Graph(_DeviceGraph):
    """Common part of GraphRRGNormal / GraphEANormal: neighbour table A[N, K], Float64 couplings J[N, K]."""
    model_kind = 5          # RRRMC_MODEL_SPARSE_F64
    energy_dtype = np.float64
    _fields_f64, _staged_thr = True, 0.8

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_graph_f64(ctx, self.A, self.J.reshape(-1)), ctx)

    def __init__(self, A, J):
        A = np.ascontiguousarray(A, np.int32)
        J = np.ascontiguousarray(J, np.float64)
        if A.ndim != 2 or A.shape != J.shape:
            raise ValueError("incompatible shapes of A and J: %r, %r" % (A.shape, J.shape))
        self.N, self.K = A.shape
        self.A, self.J = A, J

    @classmethod
    def from_AJ(cls, A, J):
        self = cls.__new__(cls)
        _SparseF64Graph.__init__(self, A, J)
        return self


class GraphRRGNormal(_SparseF64Graph):
    """``GraphRRGNormal(N, K)`` — random regular graph, couplings ~ Normal(0, 1) (src/graphs/RRG.jl:503-531).
    GRAPH stream for the pairing, one GAUSS-stream normal per bond where the reference calls ``randn()`` (RRG.jl:510-512)."""

    def __init__(self, N, K, seed=DEFAULT_SEED):
        A = np.zeros((int(N), int(K)), np.int32)
        check(lib().rrrmc_gen_rrg(N, K, seed, A))
        J = np.zeros((int(N), int(K)), np.float64)
        check(lib().rrrmc_gen_couplings_gauss(N, K, A, seed, J.reshape(-1)))
        super().__init__(A, J)


class GraphEANormal(_SparseF64Graph):
    """``GraphEANormal(L, D)`` — Edwards-Anderson lattice, couplings ~ Normal(0, 1) (src/graphs/EA.jl:534-574), or
    ``GraphEANormal(fname)`` from the text format of ``gen_AJ`` (EA.jl:73-118, D = 2):

        type: <anything>
        size: L
        name: <anything>
        x y Jxy          (one line per bond, 1-based sites)
    """

    def __init__(self, L, D=None, seed=DEFAULT_SEED):
        if isinstance(L, str):
            L, D, A, J = self._gen_AJ(L)
        else:
            if D < 1:
                raise ValueError("D must be >= 0, given: %d" % D)                  # EA.jl:566
            N = int(L) ** int(D)
            A = np.zeros((N, 2 * int(D)), np.int32)
            check(lib().rrrmc_gen_ea(L, D, A))
            J = np.zeros((N, 2 * int(D)), np.float64)
            check(lib().rrrmc_gen_couplings_gauss(N, 2 * int(D), A, seed, J.reshape(-1)))
        super().__init__(A, J)
        self.L, self.D = int(L), int(D)

    @staticmethod
    def _gen_AJ(fname):
        D = 2
        with open(fname) as f:
            if not f.readline().strip().startswith("type:"):
                raise ValueError("%s: expected a 'type:' line" % fname)
            ls = f.readline().split()
            if len(ls) != 2 or ls[0] != "size:":
                raise ValueError("%s: expected 'size: L'" % fname)
            L = int(ls[1])
            if not f.readline().strip().startswith("name:"):
                raise ValueError("%s: expected a 'name:' line" % fname)
            N = L ** D
            A = np.zeros((N, 2 * D), np.int32)
            check(lib().rrrmc_gen_ea(L, D, A))
            J = np.full((N, 2 * D), np.nan)
            for line in f:
                ls = line.split()
                if not ls:
                    continue
                if len(ls) != 3:
                    raise ValueError("%s: expected 'x y J', got %r" % (fname, line))
                x, y, Jxy = int(ls[0]) - 1, int(ls[1]) - 1, float(ls[2])
                for a, b in ((x, y), (y, x)):
                    ks = np.nonzero(A[a] == b)[0]
                    if ks.size == 0:
                        raise ValueError("%s: sites %d and %d are not neighbours" % (fname, x + 1, y + 1))
                    k = ks[0]                                                   # findfirst(Ax, y): EA.jl:99
                    if not np.isnan(J[a, k]):
                        raise ValueError("%s: bond (%d,%d) given twice" % (fname, x + 1, y + 1))
                    J[a, k] = Jxy
            if np.isnan(J).any():
                raise ValueError("%s: some bonds are missing" % fname)
        return L, D, A, J


class _DiscretizedGraph(_DeviceGraph):
    """Common part of Graph{RRG,EA}NormalDiscretized: ``A``, the Gaussian couplings ``cJ`` and their split
    ``dJ`` (levels, the inner DiscrGraph ``X0``) + ``rJ`` (residuals) by ``discretize`` (src/Common.jl:38-72)."""
    model_kind = 6          # RRRMC_MODEL_SPARSE_DISCRETIZED
    energy_dtype = np.float64

    def _upload(self, ctx):
        check(lib().rrrmc_set_graph_discretized(ctx, self.A, self.dJ, self.rJ.reshape(-1), np.asarray(self.LEV, np.int32), len(self.LEV),
                                                self.ea_form), ctx)
        check(lib().rrrmc_set_level_scale(ctx, self.lev_mul, self.lev_div), ctx)

    def _split(self, A, cJ, LEV):
        LEV = tuple(LEV)
        # Int levels: GraphRRGNormalDiscretized{Int,LEV,K}; Float64 levels -> DFloat64 (RRG.jl:324, EA.jl:357): see level_units
        self.LEV, self.lev_mul, self.lev_div = level_units(LEV)
        if max(abs(u) for u in self.LEV) > 127:
            raise NotImplementedError("levels %r need more than 8 bits per coupling after reduction by their gcd" % (LEV,))
        self.levels = LEV                                                             # as given by the caller
        if len(set(self.LEV)) != len(self.LEV):
            raise ValueError("repeated levels in LEV: %r" % (LEV,))                   # RRG.jl:100
        self.A = np.ascontiguousarray(A, np.int32)
        self.cJ = np.ascontiguousarray(cJ, np.float64)
        self.N, self.K = self.A.shape
        self.dJ = np.zeros(self.A.shape, np.int8)
        self.rJ = np.zeros(self.A.shape, np.float64)
        check(lib().rrrmc_discretize_scaled(self.cJ.reshape(-1), self.cJ.size, np.asarray(self.LEV, np.int32), len(self.LEV),
                                            self.lev_mul, self.lev_div, self.dJ.reshape(-1), self.rJ.reshape(-1)))


class GraphRRGNormalDiscretized(_DiscretizedGraph):
    """``GraphRRGNormalDiscretized(N, K, LEV)`` — DoubleGraph{DiscrGraph,Float64} (src/graphs/RRG.jl:285-324)."""
    ea_form = 0

    def __init__(self, N, K, LEV, seed=DEFAULT_SEED):
        A = np.zeros((int(N), int(K)), np.int32)
        check(lib().rrrmc_gen_rrg(N, K, seed, A))
        cJ = np.zeros((int(N), int(K)), np.float64)
        check(lib().rrrmc_gen_couplings_gauss(N, K, A, seed, cJ.reshape(-1)))
        self._split(A, cJ, LEV)


class GraphEANormalDiscretized(_DiscretizedGraph):
    """``GraphEANormalDiscretized(L, D, LEV)`` — DoubleGraph{DiscrGraph,Float64} (src/graphs/EA.jl:311-357)."""
    ea_form = 1

    def __init__(self, L, D, LEV, seed=DEFAULT_SEED):
        N = int(L) ** int(D)
        A = np.zeros((N, 2 * int(D)), np.int32)
        check(lib().rrrmc_gen_ea(L, D, A))
        cJ = np.zeros((N, 2 * int(D)), np.float64)
        check(lib().rrrmc_gen_couplings_gauss(N, 2 * int(D), A, seed, cJ.reshape(-1)))
        self._split(A, cJ, LEV)
        self.L, self.D = int(L), int(D)


class GraphSKNormal(_DeviceGraph):
    """``GraphSKNormal(N)`` — Sherrington-Kirkpatrick model, couplings ~ Normal(0, 1/N) (src/graphs/SK.jl:181-210).

    ``GraphSKNormal.from_J(J)`` is ``GraphSKNormal(J; check=true)`` (SK.jl:184-197): J must be symmetric with a
    zero diagonal.  ``ET = Float64``: energies are float64.
    """
    model_kind = 2          # RRRMC_MODEL_SK_NORMAL
    energy_dtype = np.float64
    K = 0
    _fields_f64, _staged_thr = True, 0.8

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_couplings_dense(ctx, self.J.reshape(-1)), ctx)

    def __init__(self, N, seed=DEFAULT_SEED):
        J = np.zeros((int(N), int(N)), np.float64)
        check(lib().rrrmc_gen_sk_gauss(N, seed, J.reshape(-1)))
        self.N, self.J = int(N), J

    @classmethod
    def from_J(cls, J):
        J = np.ascontiguousarray(J, np.float64)
        if J.ndim != 2 or J.shape[0] != J.shape[1]:
            raise ValueError("invalid J inner length, expected %d" % J.shape[0])
        if (np.diag(J) != 0).any():
            raise ValueError("diagonal entries of J must be 0")
        if not (J == J.T).all():
            raise ValueError("J must be symmetric")
        self = cls.__new__(cls)
        self.N, self.J = J.shape[0], J
        return self


class GraphSK(_DeviceGraph):
    """``GraphSK(N)`` — Sherrington-Kirkpatrick model with binary couplings J in {-1/sqrt(N), 1/sqrt(N)}
    (src/graphs/SK.jl:28-60).  ``J`` holds N BitVector rows ([N, ceil(N/64)] chunks, bit = 1 means +1/sqrt(N)).
    ``ET = Float64``; the cache is integer (lfields = sqrt(N) * delta_energy, SK.jl:137-140)."""
    model_kind = 4          # RRRMC_MODEL_SK_BINARY
    energy_dtype = np.float64
    K = 0
    _staged_thr = 0.8

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_couplings_bits(ctx, self.J.reshape(-1)), ctx)

    def __init__(self, N, seed=DEFAULT_SEED):
        J = np.zeros((int(N), nchunks(N)), np.uint64)
        check(lib().rrrmc_gen_sk_binary(N, seed, J.reshape(-1)))
        self.N, self.J = int(N), J


# RRRMC_RE_SLICE_* kind of a pattern machine -> the rrrmc_ctx_create_multi selector of the GraphQuant over it (RRRMC_MODEL_QUANT_PERC_STEP ...)
_QUANT_PAT_MODELS = {3: 29, 4: 30, 5: 31, 6: 32, 9: 39}


class GraphQuant(_DeviceGraph):
    """``GraphQuant(Nk, M, Γ, β, GraphRRG, Nk, K)`` — quantum Ising model in a transverse field Γ via the Suzuki-Trotter
    transformation: M coupled copies ("slices") of a classical graph (src/graphs/QT.jl:126-170).

    As the in-tree aliases do (src/QAliases.jl:43-67) the disorder is generated ONCE and shared by all slices:
    ``GraphQuant(X1, M, Γ, β)`` with ``X1`` a ``GraphRRG`` / ``GraphEA`` (±J), or a binary ``GraphSK`` — the reference's
    ``GraphQSKT(Nk, M, Γ, β)`` (src/QAliases.jl:34-43), the graph of ``scripts.jl:test_QIsing``.  ``N = Nk * M`` spins, slice-major.
    ``ET = Float64``.  ``X1`` may also be a pattern machine — ``GraphPercStep``, ``GraphPercLinear``, ``GraphCommStep``, ``GraphCommReLU``,
    ``GraphCommQu`` — whose pattern matrix all slices share: the reference's ``GraphQPercStepT`` ... (src/QAliases.jl:85-181).
    """
    model_kind = 3          # RRRMC_MODEL_QUANT_RRG
    energy_dtype = np.float64
    _rrr_classes = 4

    def _create(self, ctx, R, device, replica0):
        L = lib()
        if self.pat_slices:
            check(L.rrrmc_ctx_create_quant_pattern(ctx, self.pat_slices, self.Nk, self.K, self.M, R, device, replica0))
        elif self.sk_slices or self.skn_slices:
            check((L.rrrmc_ctx_create_quant_skn if self.skn_slices else L.rrrmc_ctx_create_quant_sk)(ctx, self.Nk, self.M, R, device, replica0))
        else:
            check((L.rrrmc_ctx_create_quant_f64 if self.f64_slices else L.rrrmc_ctx_create_quant)(ctx, self.Nk, self.K, self.M, R, device, replica0))

    def _multi_args(self):
        # a GraphQuant over other slice families is made per device by rrrmc_ctx_create_quant_skn / _sk / _f64: the header's selectors
        # RRRMC_MODEL_QUANT_SKN / _SK / _F64
        # ... and RRRMC_MODEL_QUANT_PERC_STEP / _PERC_LINEAR / _COMM_STEP / _COMM_RELU = 29 .. 32 and _COMM_QU = 39 (K = K2) for the pattern
        # machines
        if self.pat_slices:
            return _QUANT_PAT_MODELS[self.pat_slices], self.Nk, self.K, self.M
        return (9 if self.skn_slices else 8 if self.sk_slices else 10 if self.f64_slices else 3), self.Nk, self.K, self.M

    def _upload(self, ctx):
        self.X1._upload_couplings(ctx)
        check(lib().rrrmc_quant_set_field(ctx, self.beta, self.fourK), ctx)

    def __init__(self, X1, M, Gamma, beta):
        import math
        if M <= 2:
            raise ValueError("M must be greater than 2, given: %d" % M)          # QT.jl:47
        if Gamma < 0:
            raise ValueError("Γ must be >= 0")                                   # QT.jl:164
        _refuse_pspin3(X1, "GraphQuant")
        self.X1, self.M, self.Gamma, self.beta = X1, int(M), float(Gamma), float(beta)
        self.sk_slices = isinstance(X1, GraphSK)
        self.skn_slices = isinstance(X1, GraphSKNormal)                    # GraphQSKNormalT (QAliases.jl:45-46; test/runtests.jl:80)
        self.f64_slices = isinstance(X1, _SparseF64Graph)                  # GraphQEAT = GraphQuant{fourK,GraphEANormal{twoD}} (QAliases.jl:50-83)
        # pattern machines (GraphQPercStepT ..., QAliases.jl:85-159): the RRRMC_RE_SLICE_* kind; K = K2 for the committee machines
        self.pat_slices = _ensemble_slice_kind(X1) if isinstance(X1, (_GraphPerc, _GraphComm)) else 0
        dense = self.sk_slices or self.skn_slices or bool(self.pat_slices)
        self.Nk, self.K = X1.N, (X1.K if not dense or isinstance(X1, _GraphComm) else 0)
        self.N = self.Nk * self.M
        if self.pat_slices:
            self._engine = None                                            # the Engine running this graph: Renergies / Qenergy ... read its live configuration
        self.A, self.J = (None if dense else X1.A), getattr(X1, "J", None)                   # GraphSK slices: J = the bit-packed rows (SK.jl:32); GraphSKNormal: N x N Float64
        # fourK = round(2/β * log(coth(β Γ / M)), digits = MAXDIGITS): QT.jl:165
        self.fourK = round(2.0 / beta * math.log(1.0 / math.tanh(beta * Gamma / M)), 8)


def GraphQSKNormalT(Nk, M, Gamma, beta, seed=DEFAULT_SEED):
    """``GraphQSKNormalT(Nk, M, Γ, β)`` = ``GraphQuant(Nk, M, Γ, β, GraphSKNormal, SK.gen_J_gauss(Nk))`` (src/QAliases.jl:45-46)."""
    return GraphQuant(GraphSKNormal(Nk, seed=seed), M, Gamma, beta)


def _gen_J_uniform(A, seed):
    """``EA.gen_J(Float64, N, A) do 4 * rand() - 2 end`` (src/QAliases.jl:60-62 over src/graphs/EA.jl:45-71): one draw per bond x < y in (x, k) order,
    mirrored into the first free slot of row y (so that two bonds to the same neighbour — L = 2 — get two draws).  The draws come from a
    Philox generator keyed by ``seed`` (Julia's stream is not reproducible outside Julia: SURVEY.md appendix B)."""
    N, K = A.shape
    rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1)))
    J = np.full((N, K), np.nan)
    for x in range(N):
        for k in range(K):
            y = int(A[x, k])
            if x < y:
                Jxy = 4.0 * rng.random() - 2.0
                assert np.isnan(J[x, k])
                J[x, k] = Jxy
                free = np.nonzero(np.isnan(J[y]))[0]
                J[y, free[0]] = Jxy
    assert not np.isnan(J).any()
    return J


def GraphQEAT(L, D_or_M, M=None, Gamma=None, beta=None, seed=DEFAULT_SEED):
    """The reference's three constructors (src/QAliases.jl:50-83), all ``GraphQuant{fourK,GraphEANormal{2D}}`` over ONE shared ``(A, J)``:

    * ``GraphQEAT(L, D, M, Γ, β)`` — couplings uniform in [-2, 2) (``4 rand() - 2``, :60-62);
    * ``GraphQEAT(fname, M, Γ, β)`` — from the text format of ``gen_AJ`` (EA.jl:73-118);
    * ``GraphQEAT(X::GraphEANormal, M, Γ, β)``.
    """
    if isinstance(L, (str, GraphEANormal)):
        X1 = GraphEANormal(L) if isinstance(L, str) else L
        return GraphQuant(X1, D_or_M, M, Gamma)                 # (arguments shifted by one: fname | X, M, Γ, β)
    D = D_or_M
    if D < 1:
        raise ValueError("D must be ≥ 0, given: %d" % D)         # QAliases.jl:58 (the reference's message)
    N = int(L) ** int(D)
    A = np.zeros((N, 2 * int(D)), np.int32)
    check(lib().rrrmc_gen_ea(L, D, A))
    X1 = GraphEANormal.from_AJ(A, _gen_J_uniform(A, seed))
    X1.L, X1.D = int(L), int(D)
    return GraphQuant(X1, M, Gamma, beta)


def GraphQSKT(Nk, M, Gamma, beta, seed=DEFAULT_SEED):
    """``GraphQSKT(Nk, M, Γ, β)`` = ``GraphQuant(Nk, M, Γ, β, GraphSK, SK.gen_J(Nk))`` (src/QAliases.jl:34-43)."""
    return GraphQuant(GraphSK(Nk, seed=seed), M, Gamma, beta)


class _GraphPerc(_DeviceGraph):
    """The binary perceptron with ``N`` (odd) binary synapses trained on ``P`` random ±1 patterns (src/graphs/PercStep.jl, PercLinear.jl).
    ``xi`` holds the patterns as P rows of ceil(N/64) chunks, bit i of row a = ξ[a, i] (the ξv representation of gen_ξ; 1 means +1).  The
    reference draws them with an unpinned ``bitrand``: here ``seed`` names them (``rrrmc_gen_patterns``, host only), and
    ``from_patterns(ξ)`` takes an explicit P x N 0/1 matrix, as ``GraphPercStep(ξ, ξv)`` does."""
    K = 0

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create_perc(ctx, self.N, int(self.linear), R, device, replica0))

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_patterns(ctx, self.xi.reshape(-1), self.P), ctx)

    def __init__(self, N, P, seed=DEFAULT_SEED):
        N, P = int(N), int(P)
        if N % 2 == 0:
            raise ValueError("N must be odd, given: %d" % N)                             # PercStep.jl:57
        if P < 1:
            raise ValueError("P must be >= 1, given: %d" % P)
        xi = np.zeros((P, nchunks(N)), np.uint64)
        check(lib().rrrmc_gen_patterns(N, P, seed, xi.reshape(-1)))
        self.N, self.P, self.xi = N, P, xi

    @classmethod
    def from_patterns(cls, xi):
        """the graph of an explicit pattern matrix: ``xi`` is a P x N array of 0/1 (or booleans)"""
        xi = np.asarray(xi)
        if xi.ndim != 2 or xi.shape[0] < 1 or xi.shape[1] < 1:
            raise ValueError("the patterns must be a P x N matrix, given an array of shape %s" % (xi.shape,))
        if not np.isin(xi, (0, 1)).all():
            raise ValueError("the patterns must be 0/1")
        if xi.shape[1] % 2 == 0:
            raise ValueError("N must be odd, given: %d" % xi.shape[1])
        X = cls.__new__(cls)
        X.N, X.P, X.xi = int(xi.shape[1]), int(xi.shape[0]), pack_patterns(xi)
        return X

    def patterns(self):
        """the P x N matrix of 0/1"""
        return unpack_patterns(self.xi, self.N)


def pack_patterns(xi):
    """P x N 0/1 matrix -> [P, ceil(N/64)] chunks (the layout of ``rrrmc_set_patterns``)"""
    return Config.from_bits(xi).s


def unpack_patterns(chunks, N):
    """[P, ceil(N/64)] chunks -> P x N matrix of 0/1"""
    chunks = np.ascontiguousarray(chunks, np.uint64)
    if chunks.ndim != 2 or chunks.shape[1] != nchunks(N):
        raise ValueError("expected P rows of %d chunks, given an array of shape %s" % (nchunks(N), chunks.shape))
    return Config(N, chunks.shape[0], chunks).bits()


class GraphPercStep(_GraphPerc):
    """``GraphPercStep(N, P)`` (src/graphs/PercStep.jl:62-72): the energy is the number of misclassified patterns.  ``ET = Int``."""
    model_kind = 17         # RRRMC_MODEL_PERC_STEP
    energy_dtype = np.int64
    linear = False
    __doc__ += _GraphPerc.__doc__


class GraphPercLinear(_GraphPerc):
    """``GraphPercLinear(N, P)`` (src/graphs/PercLinear.jl:64-75): the energy of a pattern is the least number of synapses to flip to
    satisfy it, in units of 2 / sqrt(N).  ``ET = Float64``."""
    model_kind = 18         # RRRMC_MODEL_PERC_LINEAR
    energy_dtype = np.float64
    linear = True
    __doc__ += _GraphPerc.__doc__


class GraphPercXEntr(_DeviceGraph):
    """``GraphPercXEntr(N, P, λ)`` (src/graphs/PercXEntr.jl:74-85): the binary perceptron with the cross-entropy loss, energy
    Σ_a log(1 + exp(−2λ Δ_a / √N)) over the P patterns (Δ_a = σ·ξ_a).  ``ET = Float64``.  ``GraphPercXEntr(X, λnew)`` (:87) keeps X's patterns
    and swaps the table — annealing λ on fixed patterns.  ``from_patterns(ξ, λ)`` takes an explicit P x N 0/1 matrix.  ``xi`` holds the
    patterns in the layout of ``GraphPercStep``; ``Hs`` is the table of the N + 1 losses for Δ = −N:2:N, built here in the reference's operator
    order (:65) and handed to the library as it is (``rrrmc_set_loss_table``): given the same table the trajectory is the reference's.
    Not a slice graph of the ensembles or of GraphQuant (the reference has no such alias); ``GraphAddFields`` / ``GraphAddSubFields`` wrap
    it, which opens ``rrrMC`` on it.  See ``step_energy``."""
    K = 0
    model_kind = 66         # RRRMC_MODEL_PERC_XENTR
    energy_dtype = np.float64
    _engine = None

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create_perc_xentr(ctx, self.N, R, device, replica0))

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_patterns(ctx, self.xi.reshape(-1), self.P), ctx)
        check(lib().rrrmc_set_loss_table(ctx, self.Hs, len(self.Hs)), ctx)

    def __init__(self, N, P, lam=None, seed=DEFAULT_SEED):
        if isinstance(N, GraphPercXEntr):                                                # GraphPercXEntr(X, λnew), PercXEntr.jl:87
            if lam is not None:
                raise TypeError("expected (N, P, λ) or (X, λnew)")
            self._init(N.N, N.P, N.xi, P)
            return
        if lam is None:
            raise TypeError("expected (N, P, λ) or (X, λnew)")
        N, P = int(N), int(P)
        if N % 2 == 0:
            raise ValueError("N must be odd, given: %d" % N)                             # PercXEntr.jl:63
        if P < 1:
            raise ValueError("P must be >= 1, given: %d" % P)
        xi = np.zeros((P, nchunks(N)), np.uint64)
        check(lib().rrrmc_gen_patterns(N, P, seed, xi.reshape(-1)))
        self._init(N, P, xi, lam)

    def _init(self, N, P, xi, lam):
        if not isinstance(lam, float):
            raise TypeError("λ must be a Float64, given a %s" % type(lam).__name__)     # PercXEntr.jl:62
        self.N, self.P, self.xi, self.lam = N, P, xi, lam
        self.Hs = self.loss_table(N, lam)
        if not np.isfinite(self.Hs).all():
            raise ValueError("λ = %r at N = %d: the loss table is not finite (exp overflows)" % (lam, N))

    @staticmethod
    def loss_table(N, lam):
        """[log(1 + exp(-2 * λ * Δ / √(N))) for Δ = -N:2:N] (PercXEntr.jl:65), operator for operator; an overflowing exp is Julia's Inf"""
        import math

        def H(d):
            x = ((-2.0 * lam) * d) / math.sqrt(N)
            try:
                return math.log(1 + math.exp(x))
            except OverflowError:
                return math.inf
        return np.array([H(d) for d in range(-N, N + 1, 2)], np.float64)

    @classmethod
    def from_patterns(cls, xi, lam):
        """the graph of an explicit pattern matrix: ``xi`` is a P x N array of 0/1 (or booleans)"""
        xi = np.asarray(xi)
        if xi.ndim != 2 or xi.shape[0] < 1 or xi.shape[1] < 1:
            raise ValueError("the patterns must be a P x N matrix, given an array of shape %s" % (xi.shape,))
        if not np.isin(xi, (0, 1)).all():
            raise ValueError("the patterns must be 0/1")
        if xi.shape[1] % 2 == 0:
            raise ValueError("N must be odd, given: %d" % xi.shape[1])
        X = cls.__new__(cls)
        X._init(int(xi.shape[1]), int(xi.shape[0]), pack_patterns(xi), lam)
        return X

    def patterns(self):
        """the P x N matrix of 0/1"""
        return unpack_patterns(self.xi, self.N)


def step_energy(X, C=None):
    """``step_energy(X)`` (PercXEntr.jl:205-213): the number of misclassified patterns (Δ_a < 0) — the training error while the cross-entropy
    is being minimised — an int for one replica of the batch, shape (R,) otherwise (int64).  Read as ``LEenergies`` reads: the live
    configuration of the engine that runs ``X`` (inside a hook: the sample's), or ``C``; recomputed from the configuration on the device, so
    a hook that calls it does not change the run.  ``X`` is a ``GraphPercXEntr`` (or a field wrapper over it)."""
    E = _le_observable(X, C, "step_energy", "step_energy")
    return int(E[0]) if E.size == 1 else E


class _GraphComm(_DeviceGraph):
    """A two-layer binary committee machine: ``K2`` hidden units of ``K1`` binary synapses each, N = K1 K2 (unit k owns synapses
    k K1 .. (k + 1) K1 - 1), trained on ``P`` random ±1 patterns.  ``xi`` holds the patterns as P rows of ceil(N/64) chunks (the layout of
    ``GraphPercStep``), ``y`` (GraphCommReLU and GraphCommQu) the P labels as ceil(P/64) words.  ``fc=True`` draws each pattern over K1 inputs and
    repeats its columns K2 times (CommStep.jl:85-93).  ``seed`` names the draw (``rrrmc_gen_comm_patterns``, host only);
    ``from_patterns(K2, ξ[, y])`` takes an explicit P x N 0/1 matrix (and P labels), as ``GraphCommStep(K2, ξ, ξv)`` does."""
    relu = False

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create_comm(ctx, self.K1, self.K2, int(self.relu), R, device, replica0))

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_comm_patterns(ctx, self.K2, self.xi.reshape(-1), self.y, self.P), ctx)

    def __init__(self, K1, K2, P, fc=False, seed=DEFAULT_SEED):
        K1, K2, P = int(K1), int(K2), int(P)
        self._check_k(K1, K2)
        if P < 1:
            raise ValueError("P must be >= 1, given: %d" % P)
        xi = np.zeros((P, nchunks(K1 * K2)), np.uint64)
        y = np.zeros(nchunks(P), np.uint64) if self.relu else None
        check(lib().rrrmc_gen_comm_patterns(K1, K2, P, int(bool(fc)), seed, xi.reshape(-1), y))
        self._set(K1, K2, P, xi, y)

    @classmethod
    def _check_k(cls, K1, K2):
        par = "even" if cls.relu else "odd"
        if K1 < 1 or K1 % 2 != (0 if cls.relu else 1):
            raise ValueError("K1 must be %s, given: %d" % (par, K1))            # CommStep.jl:65-66, CommReLU.jl:68-69, CommQu.jl:72-73
        if K2 < 1 or K2 % 2 != (0 if cls.relu else 1):
            raise ValueError("K2 must be %s, given: %d" % (par, K2))

    def _set(self, K1, K2, P, xi, y):
        self.K1, self.K2, self.N, self.P, self.xi, self.y = K1, K2, K1 * K2, P, xi, y
        self.K = K2                             # the K of rrrmc_ctx_create_multi

    @classmethod
    def from_patterns(cls, K2, xi, y=None):
        """the graph of an explicit pattern matrix: ``xi`` is a P x N array of 0/1 (or booleans), N a multiple of K2; ``y`` the P labels
        (0/1) of a GraphCommReLU or GraphCommQu, and nothing for a GraphCommStep"""
        K2 = int(K2)
        xi = np.asarray(xi)
        if xi.ndim != 2 or xi.shape[0] < 1 or xi.shape[1] < 1:
            raise ValueError("the patterns must be a P x N matrix, given an array of shape %s" % (xi.shape,))
        if not np.isin(xi, (0, 1)).all():
            raise ValueError("the patterns must be 0/1")
        P, N = xi.shape
        if K2 < 1 or N % K2 != 0:
            raise ValueError("N = %d is not a multiple of K2 = %d" % (N, K2))              # CommStep.jl:61
        cls._check_k(N // K2, K2)
        if cls.relu:
            if y is None:
                raise ValueError("a %s needs the labels y" % cls.__name__)
            y = np.asarray(y)
            if y.shape != (P,):
                raise ValueError("y must hold P = %d labels, given an array of shape %s" % (P, y.shape))      # CommReLU.jl:67
            if not np.isin(y, (0, 1)).all():
                raise ValueError("the labels must be 0/1")
            y = pack_patterns(y.reshape(1, P)).reshape(-1)
        elif y is not None:
            raise ValueError("a GraphCommStep has no labels")
        X = cls.__new__(cls)
        X._set(N // K2, K2, P, pack_patterns(xi), y)
        return X

    def patterns(self):
        """the P x N matrix of 0/1"""
        return unpack_patterns(self.xi, self.N)

    def labels(self):
        """the P labels of 0/1 (GraphCommReLU, GraphCommQu); None for GraphCommStep"""
        return None if self.y is None else unpack_patterns(self.y.reshape(1, -1), self.P)[0]


class GraphCommStep(_GraphComm):
    """``GraphCommStep(K1, K2, P; fc)`` (src/graphs/CommStep.jl:73-93): hidden units with sign outputs, K1 and K2 odd; the energy is the
    number of misclassified patterns.  ``ET = Int``."""
    model_kind = 23         # RRRMC_MODEL_COMM_STEP
    energy_dtype = np.int64
    relu = False
    __doc__ += _GraphComm.__doc__


class GraphCommReLU(_GraphComm):
    """``GraphCommReLU(K1, K2, P; fc)`` (src/graphs/CommReLU.jl:76-97): hidden units with ReLU outputs, the first K2/2 with weight +1 and
    the rest −1, K1 and K2 even, and a random label per pattern; the energy is the number of misclassified patterns.  ``ET = Int``."""
    model_kind = 24         # RRRMC_MODEL_COMM_RELU
    energy_dtype = np.int64
    relu = True
    __doc__ += _GraphComm.__doc__


class GraphCommQu(_GraphComm):
    """``GraphCommQu(K1, K2, P; fc)`` (src/graphs/CommQu.jl:80-101): hidden units that answer with the square of their stability, the first
    K2/2 with weight +1 and the rest −1, K1 and K2 even, and a random label per pattern (drawn as GraphCommReLU's: CommQu.gen_ξ is
    CommReLU's); the energy is the number of misclassified patterns.  ``ET = Int``."""
    model_kind = 36         # RRRMC_MODEL_COMM_QU
    energy_dtype = np.int64
    relu = True             # even K1, K2 and labelled patterns, as GraphCommReLU
    __doc__ += _GraphComm.__doc__

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create_comm_qu(ctx, self.K1, self.K2, R, device, replica0))


class GraphSAT(_DeviceGraph):
    """``GraphSAT(N, K, α)`` (src/graphs/SAT.jl:117-127): random K-SAT with ``N`` variables and ``M = round(α N)`` clauses of ``K`` distinct
    variables each; the energy is the number of violated clauses.  ``ET = Int``.  ``A[a]`` holds the variables of clause ``a`` (0-based,
    ascending) and ``J[a]`` its literal bits: literal k is satisfied iff ``s[A[a][k]] == J[a][k]``.  ``T[i]`` lists the clauses containing
    ``i`` in clause order, ``neighb[i]`` the other variables of those clauses in order of first appearance, ``max_conn = max |T[i]|``
    (SAT.jl:86-114).  The reference draws the clauses with an unpinned ``rand``: here ``seed`` names them (``rrrmc_gen_ksat``, host only),
    and ``from_clauses(N, A, J)`` takes explicit, possibly ragged clauses (1 to 8 literals), as ``GraphSAT(N, A, J)`` does."""
    model_kind = 33         # RRRMC_MODEL_SAT
    energy_dtype = np.int64
    _staged_thr = 0.5

    def _create(self, ctx, R, device, replica0):
        check(lib().rrrmc_ctx_create_sat(ctx, self.N, R, device, replica0))

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_clauses(ctx, self.M, self.K, self._vars.reshape(-1), self._lits.reshape(-1)), ctx)

    def __init__(self, N, K, alpha, seed=DEFAULT_SEED):
        N, K = int(N), int(K)
        Mc = C.c_int64(0)
        check(lib().rrrmc_gen_ksat(N, K, float(alpha), seed, C.byref(Mc), None, None))
        vars_ = np.zeros((Mc.value, K), np.int32)
        lits = np.zeros((Mc.value, K), np.int8)
        if Mc.value:
            check(lib().rrrmc_gen_ksat(N, K, float(alpha), seed, C.byref(Mc), vars_.reshape(-1), lits.reshape(-1)))
        self._init_clauses(N, [r.tolist() for r in vars_], [r.tolist() for r in lits])

    @classmethod
    def from_clauses(cls, N, A, J):
        """the graph of explicit clauses: ``A[a]`` the 0-based variables of clause ``a`` in ascending order, ``J[a]`` its 0/1 literal bits"""
        X = cls.__new__(cls)
        X._init_clauses(int(N), [[int(i) for i in a] for a in A], [[int(j) for j in ja] for ja in J])
        return X

    def _init_clauses(self, N, A, J):
        if len(A) != len(J):
            raise ValueError("Incompatible lengths of A and J: %d vs %d" % (len(A), len(J)))      # SAT.jl:88
        if len(A) == 0:
            raise ValueError("a GraphSAT needs at least one clause")                              # (maximum over an empty collection, SAT.jl:90)
        for a, (Aa, Ja) in enumerate(zip(A, J)):
            if len(Aa) != len(Ja):
                raise ValueError("clause %d: %d variables, %d literal bits" % (a, len(Aa), len(Ja)))
            if len(Aa) == 0:
                raise ValueError("clause %d is empty" % a)
            if any(i < 0 or i >= N for i in Aa):
                raise ValueError("clause %d: a variable is out of range (N = %d)" % (a, N))
            if any(x >= y for x, y in zip(Aa, Aa[1:])):
                raise ValueError("clause %d: the variables must be distinct and in ascending order" % a)
            if any(j not in (0, 1) for j in Ja):
                raise ValueError("clause %d: literal bits must be 0 or 1" % a)
        self.N, self.M, self.K = N, len(A), max(len(a) for a in A)                                # SAT.jl:87-90
        self.A, self.J = A, J
        self.T = [[] for _ in range(N)]
        for a, Aa in enumerate(A):                                                                # SAT.jl:92-97
            for i in Aa:
                self.T[i].append(a)
        self.neighb = [[] for _ in range(N)]
        for i in range(N):                                                                        # SAT.jl:99-107
            seen = set()
            for a in self.T[i]:
                for j in A[a]:
                    if j != i and j not in seen:
                        seen.add(j)
                        self.neighb[i].append(j)
        self.max_conn = max(len(t) for t in self.T)
        self._vars = np.full((self.M, self.K), -1, np.int32)
        self._lits = np.zeros((self.M, self.K), np.int8)
        for a, (Aa, Ja) in enumerate(zip(A, J)):
            self._vars[a, :len(Aa)] = Aa
            self._lits[a, :len(Ja)] = Ja

    def export_cnf(self, path):
        """``export_cnf(X, filename)`` (SAT.jl:129-140): DIMACS CNF, variables 1-based, a positive literal where J = 1"""
        with open(path, "w") as f:
            f.write("p cnf %d %d\n" % (self.N, self.M))
            for Aa, Ja in zip(self.A, self.J):
                f.write("".join("%d " % ((2 * j - 1) * (i + 1)) for j, i in zip(Ja, Aa)) + "0\n")


class GraphPSpin3(_DeviceGraph):
    """``GraphPSpin3(N, K)`` (src/graphs/PSpin3.jl:14-53): the regular 3-spin model.  ``N`` spins, ``N`` divisible by 3; each of the ``K``
    layers is a partition of the sites into ``N / 3`` triples, all couplings +1; energy = −Σ_triples σσσ.  ``ET = Int``.  ``A[i]`` holds
    ``2K`` 0-based site ids: ``A[i][2k]``, ``A[i][2k + 1]`` are the two partners of ``i`` in layer ``k``, in the triple's own order
    (PSpin3.jl:32-43).  The reference draws the layers with an unpinned ``randperm``: here ``seed`` names them (``rrrmc_gen_pspin3``, host
    only), and ``from_triples(N, layers)`` takes explicit partitions.  ``standardMC`` runs on the graph, ``rrrMC`` on ``GraphAddFields`` /
    ``GraphAddSubFields`` over it."""
    model_kind = 105        # RRRMC_MODEL_PSPIN3
    energy_dtype = np.int64
    _staged_thr = 0.5

    def _create(self, ctx, R, device, replica0, wrap=0):
        check(lib().rrrmc_ctx_create_pspin3(ctx, self.N, self.K, wrap, R, device, replica0))

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_pspin3(ctx, self.A.reshape(-1)), ctx)

    def __init__(self, N, K, seed=DEFAULT_SEED):
        N, K = int(N), int(K)
        if K < 1:
            raise ValueError("K must be >= 1, given: %d" % K)                                     # PSpin3.jl:22
        if N < 3 or N % 3 != 0:
            raise ValueError("N must be divisible by 3, given: %d" % N)                           # PSpin3.jl:24
        A = np.zeros((N, 2 * K), np.int32)
        check(lib().rrrmc_gen_pspin3(N, K, seed, A.reshape(-1)))
        self.N, self.K, self.A = N, K, A

    @classmethod
    def from_triples(cls, N, layers):
        """the graph of explicit layers: ``layers[k]`` lists the ``N / 3`` triples ``(v1, v2, v3)`` (0-based) of layer ``k``, which must
        partition the sites; a layer may repeat"""
        N = int(N)
        if N < 3 or N % 3 != 0:
            raise ValueError("N must be divisible by 3, given: %d" % N)
        K = len(layers)
        if K < 1:
            raise ValueError("K must be >= 1, given: %d" % K)
        A = np.zeros((N, 2 * K), np.int32)
        for k, layer in enumerate(layers):
            tr = np.asarray(layer, np.int64)
            if tr.shape != (N // 3, 3):
                raise ValueError("layer %d: expected %d triples of 3 sites, given an array of shape %r" % (k, N // 3, tr.shape))
            if tr.min() < 0 or tr.max() >= N:
                raise ValueError("layer %d: a site is out of range (N = %d)" % (k, N))
            if len(np.unique(tr)) != N:
                raise ValueError("layer %d is not a partition of the sites: a site appears twice" % k)
            for v1, v2, v3 in tr.tolist():                                                        # PSpin3.jl:35-41
                A[v1, 2 * k], A[v1, 2 * k + 1] = v2, v3
                A[v2, 2 * k], A[v2, 2 * k + 1] = v1, v3
                A[v3, 2 * k], A[v3, 2 * k + 1] = v1, v2
        X = cls.__new__(cls)
        X.N, X.K, X.A = N, K, A
        return X


def _refuse_pspin3(g, what):
    """GraphPSpin3 runs stand-alone and under the field wrappers only"""
    if isinstance(g, GraphPSpin3):
        raise TypeError("%s: a GraphPSpin3 is not wired here: it runs stand-alone under standardMC, and under rrrMC as the g of "
                        "GraphAddFields / GraphAddSubFields" % what)


def _ensemble_slice_kind(slice_graph):
    if isinstance(slice_graph, GraphPSpin3):
        return 14           # RRRMC_RE_SLICE_PSPIN3 (the g of the field wrappers only)
    if isinstance(slice_graph, GraphSAT):
        return 8            # RRRMC_RE_SLICE_SAT (7 is unassigned)
    if isinstance(slice_graph, GraphCommQu):
        return 9            # RRRMC_RE_SLICE_COMM_QU
    if isinstance(slice_graph, GraphPercXEntr):
        return 11           # RRRMC_RE_SLICE_PERC_XENTR (10 is unassigned; the g of the field wrappers only)
    if isinstance(slice_graph, _SparseF64Graph):
        return 12           # RRRMC_RE_SLICE_SPARSE_F64: GraphEANormal / GraphRRGNormal slices (GraphEARE, GraphEALE, GraphEATLE)
    return (0 if slice_graph is None else 1 if isinstance(slice_graph, GraphSK) else 2 if isinstance(slice_graph, GraphSKNormal)
            else 3 if isinstance(slice_graph, GraphPercStep) else 4 if isinstance(slice_graph, GraphPercLinear)
            else 5 if isinstance(slice_graph, GraphCommStep) else 6)


def _check_sparse_slice(X1):
    """What the ensembles ask of a sparse Float64 slice graph before any device call: the rows of ``A`` ascending, in range and without
    self-loops (EA.jl:46, RRG.jl:64; ``rrrmc_set_graph_f64`` checks the same, and the symmetry of ``(A, J)``, at upload), finite couplings,
    and an even row length for a ``GraphEANormal`` (EA.jl:541-542).  Returns ``neighbors(g0, i)`` of every site: the distinct entries of
    row ``A[i]``, ascending (EA.jl:680) — D entries, not 2D, when L = 2."""
    A, J = X1.A, X1.J
    N, K = A.shape
    if isinstance(X1, GraphEANormal) and K % 2:
        raise ValueError("twoD must be even, given: %d" % K)                            # EA.jl:542
    if K < 1 or K > 8:
        raise ValueError("K = %d: the sparse Float64 slices of an ensemble take 1 <= K <= 8" % K)
    if ((A < 0) | (A >= N)).any():
        raise ValueError("invalid A, all elements must be between 1 and %d" % N)
    if (np.diff(A, axis=1) < 0).any():
        raise ValueError("invalid A, row %d is not sorted" % (int(np.nonzero((np.diff(A, axis=1) < 0).any(axis=1))[0][0]) + 1))
    if (A == np.arange(N)[:, None]).any():
        raise ValueError("invalid A, site %d neighbours itself" % (int(np.nonzero((A == np.arange(N)[:, None]).any(axis=1))[0][0]) + 1))
    if not np.isfinite(J).all():
        raise ValueError("J must be finite")
    return [[int(j) for j in np.unique(A[i])] for i in range(N)]


def _ea_slice_graph(alias, args, n_params, seed):
    """the slice graph of GraphEARE / GraphEALE / GraphEATLE and the remaining arguments: (L, D, ...) draws J = 4 rand() - 2 per bond
    (``rrrmc_gen_couplings_uniform``; src/REAliases.jl:50-59), (fname, ...) reads ``gen_AJ``'s text format, (X::GraphEANormal, ...) keeps
    ``X.A``, ``X.J`` (:61-75)"""
    if isinstance(args[0], (str, GraphEANormal)):
        if len(args) != 1 + n_params:
            raise TypeError("%s: expected (X | fname, M, ...) with %d parameters" % (alias, n_params))
        X1 = GraphEANormal(args[0]) if isinstance(args[0], str) else args[0]
        return X1, args[1:]
    if len(args) != 2 + n_params:
        raise TypeError("%s: expected (L, D, M, ...) with %d parameters" % (alias, n_params))
    L, D = args[:2]
    if D < 1:
        raise ValueError("D must be ≥ 0, given: %d" % D)                                # REAliases.jl:51 (the reference's message)
    N, K = int(L) ** int(D), 2 * int(D)
    A = np.zeros((N, K), np.int32)
    check(lib().rrrmc_gen_ea(L, D, A))
    J = np.zeros((N, K), np.float64)
    check(lib().rrrmc_gen_couplings_uniform(N, K, A, seed, -2.0, 2.0, J.reshape(-1)))
    X1 = GraphEANormal.from_AJ(A, J)
    X1.L, X1.D = int(L), int(D)
    return X1, args[2:]


def GraphEARE(*args, seed=DEFAULT_SEED):
    """``GraphEARE(L, D, M, γ, β)`` / ``GraphEARE(fname, M, γ, β)`` / ``GraphEARE(X::GraphEANormal, M, γ, β)`` (src/REAliases.jl:43-75): a
    Robust Ensemble of M replicas of one Edwards-Anderson lattice with Float64 couplings, uniform in [-2, 2) in the first form."""
    X1, (M, gamma, beta) = _ea_slice_graph("GraphEARE", args, 3, seed)
    return GraphRobustEnsemble(X1.N, M, gamma, beta, X1)


def GraphEALE(*args, seed=DEFAULT_SEED):
    """``GraphEALE(L, D, M, γ, β)`` / ``GraphEALE(fname, M, γ, β)`` / ``GraphEALE(X::GraphEANormal, M, γ, β)`` (src/LEAliases.jl:43-75): the
    Local Entropy ensemble over the same lattice; the centre and the M replicas share ``(A, J)``."""
    X1, (M, gamma, beta) = _ea_slice_graph("GraphEALE", args, 3, seed)
    return GraphLocalEntropy(X1.N, M, gamma, beta, X1)


def GraphEATLE(*args, seed=DEFAULT_SEED):
    """``GraphEATLE(L, D, M, γ, λ, β)`` / ``GraphEATLE(fname, M, γ, λ, β)`` / ``GraphEATLE(X::GraphEANormal, M, γ, λ, β)``
    (src/TLEAliases.jl:36-68): the Topological Local Entropy ensemble over the lattice; ∂i is the lattice neighbourhood of i (each
    neighbour once: D entries at L = 2)."""
    X1, (M, gamma, lam, beta) = _ea_slice_graph("GraphEATLE", args, 4, seed)
    return GraphTopologicalLocalEntropy(X1.N, M, gamma, lam, beta, X1)


def _pattern_ensemble(ens, G, sig, args, family=None, **kw):
    """the reference's two signatures (src/REAliases.jl:126-166, src/LEAliases.jl:126-189): (``sig``, M, γ, β) draws the patterns with
    ``G(sig...; kw...)``, (X, M, γ, β) takes X's.  ``family``: the class whose instances select the second signature (default: G's base, so
    that a GraphPercLinear handed to GraphPercStepRE is named in the error instead of being taken for an N)"""
    if isinstance(args[0], family or G.__base__):
        if len(args) != 4:
            raise TypeError("expected (X, M, γ, β)")
        X, M, gamma, beta = args
        if not isinstance(X, G):
            raise TypeError("expected a %s, given a %s" % (G.__name__, type(X).__name__))
    else:
        if len(args) != sig.count(",") + 4:
            raise TypeError("expected (%s, M, γ, β) or (X, M, γ, β)" % sig)
        *cargs, M, gamma, beta = args
        X = G(*cargs, **kw)
    return ens(X.N, M, gamma, beta, X)


def GraphCommStepRE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommStepRE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommStepRE(X::GraphCommStep, M, γ, β)`` (src/REAliases.jl:126-145): a Robust
    Ensemble of M committee machines that share one pattern matrix."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphCommStep, "K1, K2, P", args, fc=fc, seed=seed)


def GraphCommReLURE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommReLURE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommReLURE(X::GraphCommReLU, M, γ, β)`` (src/REAliases.jl:147-166)."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphCommReLU, "K1, K2, P", args, fc=fc, seed=seed)


def GraphCommQuRE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommQuRE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommQuRE(X::GraphCommQu, M, γ, β)`` (src/REAliases.jl:168-186)."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphCommQu, "K1, K2, P", args, fc=fc, seed=seed)


def GraphCommStepLE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommStepLE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommStepLE(X::GraphCommStep, M, γ, β)`` (src/LEAliases.jl): a Local Entropy
    ensemble of M committee machines and a centre that share one pattern matrix."""
    return _pattern_ensemble(GraphLocalEntropy, GraphCommStep, "K1, K2, P", args, fc=fc, seed=seed)


def GraphCommReLULE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommReLULE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommReLULE(X::GraphCommReLU, M, γ, β)`` (src/LEAliases.jl)."""
    return _pattern_ensemble(GraphLocalEntropy, GraphCommReLU, "K1, K2, P", args, fc=fc, seed=seed)


def GraphCommQuLE(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphCommQuLE(K1, K2, P, M, γ, β; fc)`` / ``GraphCommQuLE(X::GraphCommQu, M, γ, β)`` (src/LEAliases.jl:168-186)."""
    return _pattern_ensemble(GraphLocalEntropy, GraphCommQu, "K1, K2, P", args, fc=fc, seed=seed)


def _pattern_quant(G, sig, args, **kw):
    """the reference's two signatures (src/QAliases.jl:85-159): (``sig``, M, Γ, β) draws the patterns with ``G(sig...; kw...)``, (X, M, Γ, β)
    takes X's; ``GraphQuant`` rounds fourK to 8 digits (QT.jl:165)"""
    return _pattern_ensemble(lambda Nk, M, Gamma, beta, X: GraphQuant(X, M, Gamma, beta), G, sig, args, **kw)


def GraphQPercStepT(*args, seed=DEFAULT_SEED):
    """``GraphQPercStepT(N, P, M, Γ, β)`` / ``GraphQPercStepT(X::GraphPercStep, M, Γ, β)`` (src/QAliases.jl:101-115): a ``GraphQuant`` whose M
    Trotter slices are perceptrons on one pattern matrix — quantum annealing of a learning problem.  See ``Renergies``."""
    return _pattern_quant(GraphPercStep, "N, P", args, seed=seed)


def GraphQPercLinearT(*args, seed=DEFAULT_SEED):
    """``GraphQPercLinearT(N, P, M, Γ, β)`` / ``GraphQPercLinearT(X::GraphPercLinear, M, Γ, β)`` (src/QAliases.jl:85-99)."""
    return _pattern_quant(GraphPercLinear, "N, P", args, seed=seed)


def GraphQCommStepT(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphQCommStepT(K1, K2, P, M, Γ, β; fc)`` / ``GraphQCommStepT(X::GraphCommStep, M, Γ, β)`` (src/QAliases.jl:117-137)."""
    return _pattern_quant(GraphCommStep, "K1, K2, P", args, fc=fc, seed=seed)


def GraphQCommReLUT(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphQCommReLUT(K1, K2, P, M, Γ, β; fc)`` / ``GraphQCommReLUT(X::GraphCommReLU, M, Γ, β)`` (src/QAliases.jl:139-159)."""
    return _pattern_quant(GraphCommReLU, "K1, K2, P", args, fc=fc, seed=seed)


def GraphQCommQuT(*args, fc=False, seed=DEFAULT_SEED):
    """``GraphQCommQuT(K1, K2, P, M, Γ, β; fc)`` / ``GraphQCommQuT(X::GraphCommQu, M, Γ, β)`` (src/QAliases.jl:161-181)."""
    return _pattern_quant(GraphCommQu, "K1, K2, P", args, fc=fc, seed=seed)


def GraphSATRE(*args, seed=DEFAULT_SEED):
    """``GraphSATRE(N, K, α, M, γ, β)`` / ``GraphSATRE(X::GraphSAT, M, γ, β)`` (src/REAliases.jl:77-92): a Robust Ensemble of M replicas of
    one K-SAT instance — a replicated constraint-satisfaction problem."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphSAT, "N, K, α", args, family=GraphSAT, seed=seed)


def GraphSATLE(*args, seed=DEFAULT_SEED):
    """``GraphSATLE(N, K, α, M, γ, β)`` / ``GraphSATLE(X::GraphSAT, M, γ, β)`` (src/LEAliases.jl:77-92): a Local Entropy ensemble of M
    replicas of one K-SAT instance and a centre."""
    return _pattern_ensemble(GraphLocalEntropy, GraphSAT, "N, K, α", args, family=GraphSAT, seed=seed)


def GraphPercStepRE(*args, seed=DEFAULT_SEED):
    """``GraphPercStepRE(N, P, M, γ, β)`` / ``GraphPercStepRE(X::GraphPercStep, M, γ, β)`` (src/REAliases.jl): a Robust Ensemble of M
    perceptrons that share one pattern matrix."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphPercStep, "N, P", args, seed=seed)


def GraphPercLinearRE(*args, seed=DEFAULT_SEED):
    """``GraphPercLinearRE(N, P, M, γ, β)`` / ``GraphPercLinearRE(X::GraphPercLinear, M, γ, β)`` (src/REAliases.jl)."""
    return _pattern_ensemble(GraphRobustEnsemble, GraphPercLinear, "N, P", args, seed=seed)


def GraphPercStepLE(*args, seed=DEFAULT_SEED):
    """``GraphPercStepLE(N, P, M, γ, β)`` / ``GraphPercStepLE(X::GraphPercStep, M, γ, β)`` (src/LEAliases.jl): a Local Entropy ensemble of M
    perceptrons and a centre that share one pattern matrix."""
    return _pattern_ensemble(GraphLocalEntropy, GraphPercStep, "N, P", args, seed=seed)


def GraphPercLinearLE(*args, seed=DEFAULT_SEED):
    """``GraphPercLinearLE(N, P, M, γ, β)`` / ``GraphPercLinearLE(X::GraphPercLinear, M, γ, β)`` (src/LEAliases.jl)."""
    return _pattern_ensemble(GraphLocalEntropy, GraphPercLinear, "N, P", args, seed=seed)


# storage group of every component kind of a GraphMixed (mixed_models.hpp): a context holds one upload of each group
_MIXED_GROUPS = {1: "{SK}", 2: "{SKN}", 3: "{PERC_STEP, PERC_LINEAR, PERC_XENTR}", 4: "{PERC_STEP, PERC_LINEAR, PERC_XENTR}",
                 11: "{PERC_STEP, PERC_LINEAR, PERC_XENTR}", 5: "{COMM_STEP, COMM_RELU, COMM_QU}", 6: "{COMM_STEP, COMM_RELU, COMM_QU}",
                 9: "{COMM_STEP, COMM_RELU, COMM_QU}", 8: "{SAT}", 12: "{SPARSE_F64}"}


class _PM1AsF64:
    """A ±J ``GraphRRG`` / ``GraphEA`` (levels (-1, 1)) as a sparse Float64 component of a ``GraphMixed``: the couplings go up as ±1.0.  Every
    term of its energy and ΔE is a small integer, so the Float64 sums are the reference's integers whatever the order of additions."""

    def __init__(self, g):
        self.g, self.N, self.K = g, g.N, g.K
        self.A, self.J = g.A, np.ascontiguousarray(g.J, np.float64)
        self.energy_dtype = np.int64

    def _upload_couplings(self, ctx):
        check(lib().rrrmc_set_graph_f64(ctx, self.A, self.J.reshape(-1)), ctx)


class GraphMixed(_DeviceGraph):
    """``GraphMixed(graphs...)`` — two or more graphs on one set of spins (src/graphs/Mixed.jl:15-61): energy and delta_energy are the sums
    of the components', folded from the left in the order given (the order is part of the model: Float64 sums), ``update_cache!`` goes to
    every component.  A component is ``None`` (GraphEmpty), a ``GraphSK``, ``GraphSKNormal``, ``GraphPercStep``, ``GraphPercLinear``,
    ``GraphPercXEntr``, ``GraphCommStep``, ``GraphCommReLU``, ``GraphCommQu``, ``GraphSAT``, ``GraphRRGNormal`` / ``GraphEANormal`` (K <= 8),
    or a ±J ``GraphRRG`` / ``GraphEA`` with levels (-1, 1) and K <= 8, whose couplings are uploaded as ±1.0.  At most one component of each
    storage group ({SK}, {SKN}, the three perceptrons, the three committee machines, {SAT}, the sparse graphs): a context holds one upload
    of each.  ``standardMC`` runs on the mix, ``rrrMC`` on ``GraphAddFields`` / ``GraphAddSubFields`` over it.  ``ET`` is Int when every
    component's is, else Float64."""
    model_kind = 102        # RRRMC_MODEL_MIXED
    K = 0
    _wrap = 0
    _engine = None          # mixed_energies / step_energy read the live engine

    def __init__(self, *graphs):
        if len(graphs) < 2:
            raise ValueError("at least 2 base graphs needed")                                   # Mixed.jl:22
        if len(graphs) > 7:
            raise NotImplementedError("GraphMixed: %d components: the mixed kernels cover <= 7" % len(graphs))
        comps = []
        for g in graphs:
            _refuse_pspin3(g, "GraphMixed")
            if isinstance(g, GraphMixed):
                raise TypeError("GraphMixed: a component is a GraphMixed: a mix does not nest (list its components instead)")
            if isinstance(g, _SparseLevelsGraph):
                raise TypeError("GraphMixed: a %s with levels %r is not wired as a component (general-level graphs are not; levels (-1, 1) are)" % (type(g).__name__, g.levels))
            if isinstance(g, _DiscretizedGraph):
                raise TypeError("GraphMixed: a %s is not wired as a component (discretised graphs are not)" % type(g).__name__)
            if isinstance(g, GraphQuant):
                raise TypeError("GraphMixed: GraphQuant is not wired as a component")
            if isinstance(g, (GraphRobustEnsemble, GraphLocalEntropy, GraphTopologicalLocalEntropy)):
                raise TypeError("GraphMixed: a %s is not wired as a component (the ensembles are not)" % type(g).__name__)
            if isinstance(g, _SparsePM1Graph):
                g = _PM1AsF64(g)
            elif g is not None and not isinstance(g, (GraphSK, GraphSKNormal, _GraphPerc, GraphPercXEntr, _GraphComm, GraphSAT, _SparseF64Graph)):
                raise TypeError("GraphMixed: a %s is not wired as a component" % type(g).__name__)
            comps.append(g)
        Ns = {int(g.N) for g in comps if g is not None}
        if not Ns:
            raise ValueError("GraphMixed: at least one component must not be None (GraphEmpty), which carries no N here")
        if len(Ns) != 1:
            raise ValueError("same N for all graphs required")                                  # Mixed.jl:24
        self.N = Ns.pop()
        self.graphs = tuple(graphs)
        self._comps = tuple(comps)
        self.kinds = np.asarray([12 if isinstance(g, (_PM1AsF64, _SparseF64Graph)) else _ensemble_slice_kind(g) for g in comps], np.int32)
        seen = {}
        for c, k in enumerate(self.kinds):
            grp = _MIXED_GROUPS.get(int(k))
            if grp is None:
                continue
            if grp in seen:
                raise NotImplementedError("GraphMixed: component %d is a second graph of the storage group %s (component %d is the first): "
                                          "a context holds one upload of each group" % (c, grp, seen[grp]))
            seen[grp] = c
        self.Ksp = next((int(g.K) for g in comps if isinstance(g, (_PM1AsF64, _SparseF64Graph))), 0)
        if self.Ksp > 8:
            raise NotImplementedError("GraphMixed: K = %d: a sparse component takes 1 <= K <= 8" % self.Ksp)
        self.K2 = next((int(g.K2) for g in comps if isinstance(g, _GraphComm)), 0)
        self.energy_dtype = np.int64 if all(g is None or np.dtype(g.energy_dtype) == np.int64 for g in comps) else np.float64

    def _create(self, ctx, R, device, replica0, wrap=0):
        check(lib().rrrmc_ctx_create_mixed(ctx, self.kinds, len(self.kinds), wrap, self.N, self.Ksp, self.K2, R, device, replica0))

    def _create_multi(self, ctx, R, ids, replica0, wrap=0):
        check(lib().rrrmc_ctx_create_mixed_multi(ctx, self.kinds, len(self.kinds), wrap, self.N, self.Ksp, self.K2, R, ids, len(ids), replica0))

    def _upload_couplings(self, ctx):
        for g in self._comps:
            if g is not None:
                g._upload_couplings(ctx)


class GraphAddFields(_DeviceGraph):
    """``GraphAddFields(fields, g)`` — external fields added to a graph ``g`` (src/graphs/AddFields.jl:58-90): a DoubleGraph whose inner
    graph ``GraphAF(fields)`` has energy Σ_i h_i σ_i, delta_energy −2 σ_i h_i and no neighbours, and whose residual is ``g``'s own
    delta_energy, so that ``rrrMC`` handles the fields through its DynamicSampler at O(log N) per move whatever ``g`` is.  ``g`` is ``None``
    (GraphEmpty), a ``GraphSK``, ``GraphSKNormal``, ``GraphPercStep``, ``GraphPercLinear``, ``GraphCommStep``, ``GraphCommReLU``,
    ``GraphCommQu``, ``GraphSAT``, ``GraphPercXEntr`` or ``GraphPSpin3`` with ``len(fields)`` spins.  ``ET = Float64``: integer energies of
    ``g`` enter as exact Float64s."""
    energy_dtype = np.float64
    K = 0
    _sub = 0
    _engine = None          # step_energy over a perceptron reads the live engine

    def _create(self, ctx, R, device, replica0):
        if isinstance(self.X1, (GraphMixed, GraphPSpin3)):
            return self.X1._create(ctx, R, device, replica0, wrap=1 + self._sub)
        check(lib().rrrmc_ctx_create_af(ctx, self.slice_kind, self._sub, self.N, self.K2, R, device, replica0))

    def _multi_args(self):
        return self.model_kind, self.N, (self.X1.K if isinstance(self.X1, GraphPSpin3) else self.K2), 0

    def _create_multi(self, ctx, R, ids, replica0):
        if isinstance(self.X1, GraphMixed):
            return self.X1._create_multi(ctx, R, ids, replica0, wrap=1 + self._sub)
        _DeviceGraph._create_multi(self, ctx, R, ids, replica0)

    def _upload(self, ctx):
        if self.X1 is not None:
            self.X1._upload_couplings(ctx)
        check(lib().rrrmc_af_set_fields(ctx, self.fields), ctx)

    def __init__(self, fields, g=None):
        fields = np.ascontiguousarray(fields, np.float64)
        if fields.ndim != 1 or len(fields) < 1:
            raise ValueError("fields must be a non-empty vector")
        if g is not None and not isinstance(g, (GraphSK, GraphSKNormal, _GraphPerc, _GraphComm, GraphSAT, GraphPercXEntr, GraphMixed, GraphPSpin3)):
            raise TypeError("%s wraps GraphEmpty (None), GraphSK, GraphSKNormal, GraphPercStep, GraphPercLinear, GraphCommStep, GraphCommReLU, "
                            "GraphCommQu, GraphSAT, GraphPercXEntr, GraphPSpin3 or a GraphMixed of them; sparse graphs (GraphRRG*, GraphEA*), GraphQuant and the ensembles are not wired as g, "
                            "given a %s" % (type(self).__name__, type(g).__name__))
        if g is not None and g.N != len(fields):
            raise ValueError("incompatible length, fields size=%d graph size=%d" % (len(fields), g.N))       # AddFields.jl:65
        if not np.all(np.isfinite(fields)):
            raise ValueError("the fields must be finite")
        self.fields, self.N, self.X1 = fields, len(fields), g
        if isinstance(g, GraphMixed):
            self.slice_kind, self.K2 = 13, g.K2                                                               # RRRMC_RE_SLICE_MIXED
            self.model_kind = 104 if self._sub else 103                                                       # RRRMC_MODEL_MIXED_ASF / _MIXED_AF
            return
        self.slice_kind = _ensemble_slice_kind(g)
        self.K2 = int(getattr(g, "K2", 0)) if isinstance(g, _GraphComm) else 0
        if self.slice_kind == 14:
            self.model_kind = 107 if self._sub else 106                                                       # RRRMC_MODEL_PSPIN3_ASF / _AF
        elif self.slice_kind == 11:
            self.model_kind = 101 if self._sub else 100                                                       # RRRMC_MODEL_XENTR_ASF / _AF
        else:
            self.model_kind = (57 if self._sub else 48) + (0, 1, 2, 3, 4, 5, 6, None, 7, 8)[self.slice_kind]  # RRRMC_MODEL_AF_* / RRRMC_MODEL_ASF_*


class GraphAddSubFields(GraphAddFields):
    """``GraphAddSubFields(fields, g)`` — the fields added and subtracted (src/graphs/AddFields.jl:94-123): energy and delta_energy are
    ``g``'s own, the residual is ``delta_energy(g) − delta_energy(GraphAF(fields))``.  The fields only shape the proposals of ``rrrMC``;
    the stationary law is ``g``'s."""
    _sub = 1


class GraphRobustEnsemble(_DeviceGraph):
    """``GraphRobustEnsemble(Nk, M, γ, β, slice_graph)`` — the Robust Ensemble (src/graphs/RE.jl:215-263): M replicas of one graph (the
    slices, which share one coupling set as ``Gconstr(args...)`` with the same ``args`` gives them) coupled by ``GraphRE{M,γ,β}`` through
    μ_i = Σ_k σ_(i,k), energy Σ_i −log(2 cosh(γ μ_i)) / β.  ``slice_graph`` is ``None`` (GraphEmpty: ``Graph0RE``), a binary ``GraphSK``
    (``GraphSKRE``) or a ``GraphSKNormal`` with ``N == Nk``.  ``N = Nk * M`` spins in the reference's order: site j is spin j // M of replica
    j % M (RE.jl:76-95).  β here is the graph's (inside fk), not a sampler's.  ``ET = Float64``.  See ``REenergies``."""
    energy_dtype = np.float64
    K = 0
    _rrr_classes = property(lambda self: 2 * ((self.M + 1) // 2))

    def _create(self, ctx, R, device, replica0):
        if self.slice_kind == 12:          # sparse Float64 slices: the creator that carries K
            check(lib().rrrmc_ctx_create_re_f64(ctx, self.Nk, self.K, self.M, R, device, replica0))
        else:
            check(lib().rrrmc_ctx_create_re(ctx, self.Nk, self.M, self.slice_kind, R, device, replica0))

    def _multi_args(self):
        return self.model_kind, self.Nk, self.K, self.M

    def _upload(self, ctx):
        if self.X1 is not None:
            self.X1._upload_couplings(ctx)
        check(lib().rrrmc_re_set_params(ctx, self.gamma, self.beta), ctx)

    def __init__(self, Nk, M, gamma, beta, slice_graph=None):
        if M <= 2:
            raise ValueError("M must be greater than 2, given: %d" % M)                  # RE.jl:37
        _refuse_pspin3(slice_graph, "GraphRobustEnsemble")
        if slice_graph is not None and not isinstance(slice_graph, (GraphSK, GraphSKNormal, _GraphPerc, _GraphComm, GraphSAT, _SparseF64Graph)):
            raise TypeError("the slices of a GraphRobustEnsemble are GraphEmpty (None), GraphSK, GraphSKNormal, GraphPercStep, GraphPercLinear, "
                            "GraphCommStep, GraphCommReLU, GraphCommQu, GraphSAT, GraphEANormal or GraphRRGNormal")
        if slice_graph is not None and slice_graph.N != int(Nk):
            raise ValueError("the slice graph has %d spins, expected Nk = %d" % (slice_graph.N, Nk))
        self.Nk, self.M, self.gamma, self.beta = int(Nk), int(M), float(gamma), float(beta)
        self.N = self.Nk * self.M
        self.X1 = slice_graph
        self.slice_kind = _ensemble_slice_kind(slice_graph)
        self.model_kind = (11, 12, 13, 19, 20, 25, 26, None, 34, 37, None, None, 67)[self.slice_kind]  # RRRMC_MODEL_RE_EMPTY / _SK / _SKN / _PERC_* / _COMM_* / _SAT / _COMM_QU / _SPARSE_F64
        if self.slice_kind == 12:
            _check_sparse_slice(slice_graph)
            self.K = slice_graph.K                      # rrrmc_ctx_create_re_f64 and rrrmc_ctx_create_multi carry the slice graph's K
        self.J = getattr(slice_graph, "J", None)
        self._engine = None                             # the Engine running this graph: REenergies reads the live configuration there

    def tables(self):
        """(ΔElist[M], μ-energies[M + 1]) of GraphRE{M,γ,β} (rrrmc_re_tables: host libm, no device)"""
        dE = np.zeros(self.M, np.float64)
        e0 = np.zeros(self.M + 1, np.float64)
        check(lib().rrrmc_re_tables(self.M, self.gamma, self.beta, dE, e0))
        return dE, e0


def Graph0RE(Nk, M, gamma, beta):
    """``Graph0RE(Nk, M, γ, β)`` = ``GraphRobustEnsemble(Nk, M, γ, β, GraphEmpty, Nk)`` (src/REAliases.jl:20-29)."""
    return GraphRobustEnsemble(Nk, M, gamma, beta, None)


def GraphSKRE(Nk, M, gamma, beta, seed=DEFAULT_SEED):
    """``GraphSKRE(Nk, M, γ, β)`` = ``GraphRobustEnsemble(Nk, M, γ, β, GraphSK, SK.gen_J(Nk))`` (src/REAliases.jl:33-38): the couplings are
    drawn once (``rrrmc_gen_sk_binary``, as ``GraphSK`` does) and shared by the M slices."""
    return GraphRobustEnsemble(Nk, M, gamma, beta, GraphSK(Nk, seed=seed))


def REenergies(X, C=None):
    """``REenergies(X)`` (RE.jl:285-301): the energy of every replica of the ensemble as its own graph defines it — shape (M,) for one
    replica of the batch, (R, M) otherwise — computed on the device from the CURRENT configuration of the engine that runs ``X`` (inside a
    hook: the sample's configuration).  With ``C`` (a ``Config`` of N = Nk M spins) it is evaluated for that configuration instead."""
    return _le_observable(X, C, "REenergies", "re_energies")


class GraphLocalEntropy(_DeviceGraph):
    """``GraphLocalEntropy(Nk, M, γ, β, slice_graph)`` — the Local Entropy ensemble (src/graphs/LE.jl:183-318): M replicas of one graph (the
    slices), each coupled to an explicit reference configuration (the "centre", under a graph of the same kind, all sharing one coupling set)
    by ``GraphLE{M,γT}`` with γT = γ / β: ΔE0 = 2γT σc σ_(i,k) on a replica site and 2γT σc μ_i (μ_i = Σ_k σ_(i,k)) on the centre.
    ``slice_graph`` is ``None`` (GraphEmpty: ``Graph0LE``), a binary ``GraphSK`` (``GraphSKLE``) or a ``GraphSKNormal`` with ``N == Nk``.
    ``N = Nk * (M + 1)`` spins in the reference's order: site j is spin j // (M+1) of the centre when j % (M+1) == 0 and of replica j % (M+1)
    otherwise (LE.jl:55-84).  β here is the graph's (γT = γ / β), not a sampler's.  ``ET = Float64``.  The centre's own energy is not part
    of the ensemble's energy.  See ``LEenergies``, ``cenergy`` and ``distances``."""
    energy_dtype = np.float64
    K = 0
    _rrr_classes = property(lambda self: 2 * (self.M // 2 + 2 if self.M % 2 == 0 else (self.M + 1) // 2))

    def _create(self, ctx, R, device, replica0):
        if self.slice_kind == 12:          # sparse Float64 slices: the creator that carries K
            check(lib().rrrmc_ctx_create_le_f64(ctx, self.Nk, self.K, self.M, R, device, replica0))
        else:
            check(lib().rrrmc_ctx_create_le(ctx, self.Nk, self.M, self.slice_kind, R, device, replica0))

    def _multi_args(self):
        return self.model_kind, self.Nk, self.K, self.M

    def _upload(self, ctx):
        if self.X1 is not None:
            self.X1._upload_couplings(ctx)
        check(lib().rrrmc_le_set_params(ctx, self.gamma, self.beta), ctx)

    def __init__(self, Nk, M, gamma, beta, slice_graph=None):
        if M <= 2:
            raise ValueError("M must be greater than 2, given: %d" % M)                  # LE.jl:24
        _refuse_pspin3(slice_graph, "GraphLocalEntropy")
        if slice_graph is not None and not isinstance(slice_graph, (GraphSK, GraphSKNormal, _GraphPerc, _GraphComm, GraphSAT, _SparseF64Graph)):
            raise TypeError("the slices of a GraphLocalEntropy are GraphEmpty (None), GraphSK, GraphSKNormal, GraphPercStep, GraphPercLinear, "
                            "GraphCommStep, GraphCommReLU, GraphCommQu, GraphSAT, GraphEANormal or GraphRRGNormal")
        if slice_graph is not None and slice_graph.N != int(Nk):
            raise ValueError("the slice graph has %d spins, expected Nk = %d" % (slice_graph.N, Nk))
        self.Nk, self.M, self.gamma, self.beta = int(Nk), int(M), float(gamma), float(beta)
        self.gammaT = self.gamma / self.beta                                              # LE.jl:221-225
        self.N = self.Nk * (self.M + 1)
        self.X1 = slice_graph
        self.slice_kind = _ensemble_slice_kind(slice_graph)
        self.model_kind = (14, 15, 16, 21, 22, 27, 28, None, 35, 38, None, None, 68)[self.slice_kind]  # RRRMC_MODEL_LE_EMPTY / _SK / _SKN / _PERC_* / _COMM_* / _SAT / _COMM_QU / _SPARSE_F64
        if self.slice_kind == 12:
            _check_sparse_slice(slice_graph)
            self.K = slice_graph.K                      # rrrmc_ctx_create_le_f64 and rrrmc_ctx_create_multi carry the slice graph's K
        self.J = getattr(slice_graph, "J", None)
        self._engine = None                             # the Engine running this graph: the observables read the live configuration there

    def tables(self):
        """allΔE of GraphLE{M,γT} (rrrmc_le_tables: host only, no device)"""
        L = self.M // 2 + 2 if self.M % 2 == 0 else (self.M + 1) // 2
        dE = np.zeros(L, np.float64)
        check(lib().rrrmc_le_tables(self.M, self.gamma, self.beta, dE))
        return dE


def Graph0LE(Nk, M, gamma, beta):
    """``Graph0LE(Nk, M, γ, β)`` = ``GraphLocalEntropy(Nk, M, γ, β, GraphEmpty, Nk)`` (src/LEAliases.jl)."""
    return GraphLocalEntropy(Nk, M, gamma, beta, None)


def GraphSKLE(Nk, M, gamma, beta, seed=DEFAULT_SEED):
    """``GraphSKLE(Nk, M, γ, β)`` = ``GraphLocalEntropy(Nk, M, γ, β, GraphSK, SK.gen_J(Nk))`` (src/LEAliases.jl): the couplings are drawn once
    (``rrrmc_gen_sk_binary``, as ``GraphSK`` does) and shared by the centre and the M slices."""
    return GraphLocalEntropy(Nk, M, gamma, beta, GraphSK(Nk, seed=seed))


def _tle_check_neighb(Nk, M, neighb):
    """the checks of GraphTLE's constructor (TLE.jl:27-46), 0-based lists; the messages carry the reference's 1-based numbers"""
    if M <= 2:
        raise ValueError("M must be greater than 2, given: %d" % M)                      # TLE.jl:29
    if len(neighb) != Nk:
        raise ValueError("invalid neighb argument, expected length %d, given: %d" % (Nk, len(neighb)))
    for i, ni in enumerate(neighb):
        if not all(0 <= j < Nk for j in ni):
            raise ValueError("invalid neighb[%d] argument, all elements must be between 1 and %d" % (i + 1, Nk))
        if i in ni:
            raise ValueError("invalid neighb[%d], contains itself" % (i + 1))
        for i1 in range(len(ni)):
            if ni[i1] in ni[i1 + 1:]:
                raise ValueError("duplicated element %d in neighb[%d]" % (i1 + 1, i + 1))
    sets = [set(ni) for ni in neighb]
    for i, ni in enumerate(neighb):
        for i1 in ni:
            if i not in sets[i1]:
                raise ValueError("neighb is not symmetrical, %d ∈ ∂%d but %d ∉ ∂%d" % (i1 + 1, i + 1, i + 1, i1 + 1))


class GraphTopologicalLocalEntropy(_DeviceGraph):
    """``GraphTopologicalLocalEntropy(Nk, M, γ, λ, β, slice_graph)`` — the Local Entropy ensemble with a topological interaction
    (src/graphs/TLE.jl:351-396): as ``GraphLocalEntropy``, M replicas of one graph and a centre, coupled by ``GraphTLE{M,γT,λT}`` with
    γT = γ / β and λT = λ / β: ΔE0 = 2γT lfields1 + 2λT lfields2, where lfields1 is GraphLE's field and lfields2 on replica site (i,k) is
    σ_(i,k) σc_i Σ_{i2 ∈ ∂i} σc_i2 σ_(i2,k) (on a centre: the sum of its replicas').  ∂i = ``neighb[i]`` is ``neighbors(slice_graph, i)``:
    empty for ``None`` (GraphEmpty: ``Graph0TLE``), all other sites ascending for a binary ``GraphSK`` (``GraphSKTLE``) or a
    ``GraphSKNormal``, ``GraphSAT.neighb`` for a ``GraphSAT`` (``GraphSATTLE``).  Sites, their order and the observables are
    ``GraphLocalEntropy``'s.  ``ET = Float64``.  See ``TLEenergies``, ``cenergy`` and ``distances``."""
    energy_dtype = np.float64
    K = 0

    def _create(self, ctx, R, device, replica0):
        if self.slice_kind == 12:          # sparse Float64 slices: the creator that carries K
            check(lib().rrrmc_ctx_create_tle_f64(ctx, self.Nk, self.K, self.M, R, device, replica0))
        else:
            check(lib().rrrmc_ctx_create_tle(ctx, self.Nk, self.M, self.slice_kind, R, device, replica0))

    def _multi_args(self):
        return self.model_kind, self.Nk, self.K, self.M

    def _upload(self, ctx):
        if self.X1 is not None:
            self.X1._upload_couplings(ctx)
        check(lib().rrrmc_tle_set_topology(ctx, self._rowptr, self._cols), ctx)
        check(lib().rrrmc_tle_set_params(ctx, self.gamma, self.lam, self.beta), ctx)

    def __init__(self, Nk, M, gamma, lam, beta, slice_graph=None):
        _refuse_pspin3(slice_graph, "GraphTopologicalLocalEntropy")
        if slice_graph is not None and not isinstance(slice_graph, (GraphSK, GraphSKNormal, GraphSAT, _SparseF64Graph)):
            raise TypeError("the slices of a GraphTopologicalLocalEntropy are GraphEmpty (None), GraphSK, GraphSKNormal, GraphSAT, GraphEANormal or GraphRRGNormal")
        if slice_graph is not None and slice_graph.N != int(Nk):
            raise ValueError("expected %d spins, got %d" % (Nk, slice_graph.N))           # TLE.jl:392
        self.Nk, self.M, self.gamma, self.lam, self.beta = int(Nk), int(M), float(gamma), float(lam), float(beta)
        if slice_graph is None:
            neighb = [[] for _ in range(self.Nk)]
        elif isinstance(slice_graph, GraphSAT):
            neighb = [list(ni) for ni in slice_graph.neighb]
        elif isinstance(slice_graph, _SparseF64Graph):
            neighb = _check_sparse_slice(slice_graph)                                     # uA[i]: neighbors(g0, i), EA.jl:680, TLE.jl:394
            self.K = slice_graph.K
        else:
            neighb = [[j for j in range(self.Nk) if j != i] for i in range(self.Nk)]      # AllButOne
        _tle_check_neighb(self.Nk, self.M, neighb)
        self.neighb = neighb
        self.gammaT, self.lambdaT = self.gamma / self.beta, self.lam / self.beta           # TLE.jl:390-396
        self.N = self.Nk * (self.M + 1)
        self.X1 = slice_graph
        self.slice_kind = _ensemble_slice_kind(slice_graph)
        self.model_kind = {0: 44, 1: 45, 2: 46, 8: 47, 12: 69}[self.slice_kind]           # RRRMC_MODEL_TLE_EMPTY / _SK / _SKN / _SAT / _SPARSE_F64
        self.J = getattr(slice_graph, "J", None)
        self.max_deg = max(len(ni) for ni in neighb)
        self._rowptr = np.zeros(self.Nk + 1, np.int32)
        self._rowptr[1:] = np.cumsum([len(ni) for ni in neighb])
        self._cols = np.array([j for ni in neighb for j in ni] or [0], np.int32)
        self._engine = None                             # the Engine running this graph: the observables read the live configuration there

    def tables(self):
        """allΔE of GraphTLE{M,γT,λT} (rrrmc_tle_tables: host only, no device)"""
        L = C.c_int64(0)
        check(lib().rrrmc_tle_tables(self.M, self.gamma, self.lam, self.beta, self.max_deg, None, C.byref(L)))
        dE = np.zeros(L.value, np.float64)
        check(lib().rrrmc_tle_tables(self.M, self.gamma, self.lam, self.beta, self.max_deg, dE.ctypes.data, C.byref(L)))
        return dE

    _rrr_classes = property(lambda self: 2 * len(self.tables()))


def Graph0TLE(Nk, M, gamma, lam, beta):
    """``Graph0TLE(Nk, M, γ, λ, β)`` = ``GraphTopologicalLocalEntropy(Nk, M, γ, λ, β, GraphEmpty, Nk)`` (src/TLEAliases.jl): no neighbours,
    so the model coincides with ``Graph0LE(Nk, M, γ, β)``."""
    return GraphTopologicalLocalEntropy(Nk, M, gamma, lam, beta, None)


def GraphSKTLE(Nk, M, gamma, lam, beta, seed=DEFAULT_SEED):
    """``GraphSKTLE(Nk, M, γ, λ, β)`` = ``GraphTopologicalLocalEntropy(Nk, M, γ, λ, β, GraphSK, SK.gen_J(Nk))`` (src/TLEAliases.jl): the
    couplings are drawn once and shared by the centre and the M slices; every site neighbours every other."""
    return GraphTopologicalLocalEntropy(Nk, M, gamma, lam, beta, GraphSK(Nk, seed=seed))


def GraphSATTLE(*args, seed=DEFAULT_SEED):
    """``GraphSATTLE(N, K, α, M, γ, λ, β)`` / ``GraphSATTLE(X::GraphSAT, M, γ, λ, β)`` (src/TLEAliases.jl): a Topological Local Entropy
    ensemble of M replicas of one K-SAT instance and a centre; two variables are neighbours when they share a clause."""
    if isinstance(args[0], GraphSAT):
        if len(args) != 5:
            raise TypeError("expected (X, M, γ, λ, β)")
        X, M, gamma, lam, beta = args
    else:
        if len(args) != 7:
            raise TypeError("expected (N, K, α, M, γ, λ, β) or (X, M, γ, λ, β)")
        *cargs, M, gamma, lam, beta = args
        X = GraphSAT(*cargs, seed=seed)
    return GraphTopologicalLocalEntropy(X.N, M, gamma, lam, beta, X)


def TLEenergies(X, C=None):
    """``TLEenergies(X)`` (TLE.jl:437-453): the energy of every replica of the ensemble as its own graph defines it; shapes and reading
    as ``LEenergies``."""
    return _le_observable(X, C, "TLEenergies", "le_energies")


def _le_observable(X, C, name, fn):
    from .engine import Engine
    if C is not None:
        with Engine(X, C.R) as eng:
            eng.set_config(C)
            return getattr(eng, fn)()
    eng = getattr(X, "_engine", None)
    if eng is None or not eng._ctx:
        raise RuntimeError("%s(X): no engine is running this graph; pass a configuration: %s(X, C)" % (name, name))
    return getattr(eng, fn)()


def LEenergies(X, C=None):
    """``LEenergies(X)`` (LE.jl:259-269): the energy of every replica of the ensemble as its own graph defines it — shape (M,) for one
    replica of the batch, (R, M) otherwise — computed on the device from the CURRENT configuration of the engine that runs ``X`` (inside a
    hook: the sample's configuration).  With ``C`` (a ``Config`` of N = Nk (M+1) spins) it is evaluated for that configuration instead.
    Unlike the reference's, it reads the configuration only (the slice caches are not rebuilt): a hook that calls it does not change the run."""
    return _le_observable(X, C, "LEenergies", "le_energies")


def cenergy(X, C=None):
    """``cenergy(X)`` (LE.jl:271-274): the energy of the centre configuration under the slice graph (0 for GraphEmpty) — a float for one
    replica of the batch, shape (R,) otherwise; read as ``LEenergies`` reads (the live engine, or ``C``), without rebuilding any cache."""
    return _le_observable(X, C, "cenergy", "cenergy")


def distances(X, C=None):
    """``distances(X)`` (LE.jl:309-318): the M x M matrix of Hamming distances between the replica configurations, centre excluded — shape
    (M, M) for one replica of the batch, (R, M, M) otherwise (int64); read as ``LEenergies`` reads."""
    return _le_observable(X, C, "distances", "distances")


def Renergies(X, C=None):
    """``Renergies(X)`` (QT.jl:201-211) of a ``GraphQuant`` over pattern machines: the energy of every Trotter slice under its own graph — the
    training errors; their minimum is what a quantum-annealing run on a learning problem reports — shape (M,) for one replica of the batch,
    (R, M) otherwise.  Read as ``LEenergies`` reads: the live configuration of the engine that runs ``X`` (inside a hook: the sample's), or
    ``C``; recomputed from the configuration on the device, so a hook that calls it does not change the run."""
    return _le_observable(X, C, "Renergies", "quant_renergies")


def Qenergy(X, C=None):
    """``Qenergy(X, C)`` (QT.jl:253-268) of a ``GraphQuant``: a float for one replica of the batch, shape (R,) otherwise; read as ``Renergies``."""
    Q = _le_observable(X, C, "Qenergy", "quant_observables")[0]
    return float(Q[0]) if Q.size == 1 else Q


def transverse_mag(X, C=None, beta=None):
    """``transverse_mag(X.X0, C, β)`` (QT.jl:113-122) of a ``GraphQuant`` (β defaults to the graph's): a float for one replica, else (R,)."""
    tm = _le_observable(X, C, "transverse_mag", "quant_observables")[1] if beta is None else _quant_observables_at(X, C, beta)[1]
    return float(tm[0]) if tm.size == 1 else tm


def overlaps(X, C=None):
    """``overlaps(X)`` (QT.jl:213-251) of a ``GraphQuant``: shape (M // 2,) for one replica of the batch, (R, M // 2) otherwise."""
    ov = _le_observable(X, C, "overlaps", "quant_observables")[2]
    return ov[0] if ov.shape[0] == 1 else ov


def _quant_observables_at(X, C, beta):
    from .engine import Engine
    if C is not None:
        with Engine(X, C.R) as eng:
            eng.set_config(C)
            return eng.quant_observables(beta=beta)
    eng = getattr(X, "_engine", None)
    if eng is None or not eng._ctx:
        raise RuntimeError("transverse_mag(X): no engine is running this graph; pass a configuration")
    return eng.quant_observables(beta=beta)


def checkerboard_coloring(L, D):
    """Two-colouring (parity of the coordinate sum) of the periodic L^D lattice of ``GraphEA``; L must be even."""
    if L % 2:
        raise ValueError("the periodic lattice is two-colourable only for even L, given: %d" % L)
    x = np.arange(int(L) ** int(D))
    par = np.zeros_like(x)
    for d in range(int(D)):
        par += (x // int(L) ** d) % int(L)
    return (par % 2).astype(np.int32)


def getN(X):
    """src/Interface.jl:145"""
    return X.N


def neighbors(X, i):
    """src/Interface.jl:158; RRG.jl:261 (uA = neighbours with non-zero coupling), EA.jl:292 (de-duplicated)."""
    if isinstance(X, GraphPSpin3):
        a = X.A[i]
        return a[np.sort(np.unique(a, return_index=True)[1])].astype(np.int64)                     # unique(A[i]), first occurrences in order: PSpin3.jl:47, :177
    if isinstance(X, GraphSAT):
        return np.asarray(X.neighb[i], np.int64)                                                  # SAT.jl:322
    if getattr(X, "model_kind", 0) == 7 and not X.ea_form:
        return X.A[i][X.J[i] != 0]
    return np.unique(X.A[i])


def all_delta_e(X):
    """allΔE (src/Interface.jl:200-201): RRG.jl:262-281, EA.jl:293-309 — sorted values of |dE|."""
    if isinstance(X, GraphSAT):
        return tuple(range(X.max_conn + 1))                                                       # SAT.jl:325
    if isinstance(X, GraphPSpin3):                                                                # PSpin3.jl:178-180
        K = X.K
        return tuple(4 * d for d in range(K // 2 + 1)) if K % 2 == 0 else tuple(2 * (2 * d + 1) for d in range((K + 1) // 2))
    K = X.K
    if getattr(X, "model_kind", 0) == 7:
        es = {0}
        for _ in range(K):
            es = {e + s * l for e in es for l in X.LEV for s in (-1, 1)}
        return tuple(X.energy_value(sorted({2 * abs(e) for e in es})).tolist())
    return tuple(2 * m for m in range(K & 1, K + 1, 2))
