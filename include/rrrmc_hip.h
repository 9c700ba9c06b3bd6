/*
 * rrrmc_hip.h — C ABI of the MI355X (gfx950) Ising Monte Carlo sweep engine.
 *
 * This is the drop-in boundary behind RRRMC.jl's AbstractGraph / standardMC API.
 * In the reference the samplers call the graph through a per-site interface
 * (src/Interface.jl:87-158: energy, delta_energy, spinflip!/update_cache!, neighbors, allΔE);
 * a per-site call across an FFI is useless on a GPU, so the boundary sits one level up: one call
 * runs the WHOLE sampler loop (src/RRRMC.jl:81-127) for a batch of R replicas of one graph.
 *
 * Conventions
 *  - every function returns an int32 status (RRRMC_OK == 0); the text of the last failure is
 *    available from rrrmc_last_error(ctx) (ctx may be NULL for creation failures);
 *    nothing throws or aborts across the ABI (the reference raises ArgumentError, src/RRRMC.jl:94).
 *  - the caller owns every host buffer and keeps it alive for the duration of the call
 *    (Julia: GC.@preserve); the library owns all device memory inside the ctx.
 *  - spins travel in Julia's BitVector chunk layout (src/Interface.jl:21-29, src/Common.jl:15-23):
 *    replica r, site x (0-based) = bit (x & 63) of chunks[r * nchunks + (x >> 6)], nchunks = ceil(N/64);
 *    spin value sigma = 2*bit - 1.  Unused high bits of the last chunk are zero.
 *  - neighbour tables are row-major N x K, 0-BASED int32 (the Julia glue subtracts 1 from
 *    reinterpret(Int64, X.A), src/graphs/RRG.jl:118-119); couplings are N x K int8 (+-1).
 *  - a ctx made by rrrmc_ctx_create is bound to ONE device; rrrmc_ctx_create_multi spreads the replicas of one ctx over several
 *    (one stream and one host thread per device).  No ctx is re-entrant (the reference's graph objects are stateful too:
 *    src/graphs/RRG.jl:121).  A multi-process job instead gives every process its own ctx with a replica offset.
 *  - random numbers: Philox4x32-10 streams addressed by (seed; iteration, replica) — see DESIGN.md
 *    "Random-stream contract"; results do not depend on how replicas are sharded over devices.
 */
#ifndef RRRMC_HIP_H
#define RRRMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRRMC_API __attribute__((visibility("default")))

typedef struct rrrmc_ctx rrrmc_ctx;

enum rrrmc_status {
    RRRMC_OK = 0,
    RRRMC_ERR_INVALID_ARG = 1,   /* reference: ArgumentError */
    RRRMC_ERR_STATE = 2,         /* call order violated (e.g. sampling before set_graph) */
    RRRMC_ERR_UNSUPPORTED = 3,   /* model/size outside what the HIP kernels cover */
    RRRMC_ERR_HIP = 4,           /* HIP runtime failure (no device, launch error, ...) */
    RRRMC_ERR_NOMEM = 5
};

enum rrrmc_model {
    RRRMC_MODEL_SPARSE_PM1 = 1,  /* GraphRRG{Int,(-1,1),K} src/graphs/RRG.jl:116 and GraphEA{Int,(-1,1),2D} src/graphs/EA.jl:138 */
    RRRMC_MODEL_SK_NORMAL = 2,   /* GraphSKNormal (Float64 couplings) src/graphs/SK.jl:181-210; K is ignored */
    RRRMC_MODEL_SPARSE_F64 = 5,  /* GraphRRGNormal{K} src/graphs/RRG.jl:503-520 and GraphEANormal{2D} src/graphs/EA.jl:534-552: sparse, Float64 couplings */
    RRRMC_MODEL_SPARSE_DISCRETIZED = 6, /* GraphRRGNormalDiscretized src/graphs/RRG.jl:285-307, GraphEANormalDiscretized src/graphs/EA.jl:311-352 (Int or DFloat64 LEV) */
    RRRMC_MODEL_SPARSE_LEVELS = 7,      /* GraphRRG{ET,LEV,K} src/graphs/RRG.jl:116-162, GraphEA{ET,LEV,2D} src/graphs/EA.jl:138-193 with levels other than (-1,1); ET = Int or DFloat64 */
    RRRMC_MODEL_SK_BINARY = 4,   /* GraphSK (couplings +-1/sqrt(N), bit-packed) src/graphs/SK.jl:28-60; K is ignored; energies Float64 */
    RRRMC_MODEL_QUANT_RRG = 3,   /* GraphQuant over M Suzuki-Trotter slices of one GraphRRG{Int,(-1,1),K} disorder
                                    (src/graphs/QT.jl:126-170 with the shared-disorder pattern of src/QAliases.jl:43-67);
                                    created with rrrmc_ctx_create_quant */
    /* selectors for rrrmc_ctx_create_multi only (the contexts it makes report RRRMC_MODEL_QUANT_RRG): */
    RRRMC_MODEL_QUANT_SK = 8,    /* GraphQuant over binary GraphSK slices (GraphQSKT, src/QAliases.jl:34-43): rrrmc_ctx_create_quant_sk per device */
    RRRMC_MODEL_QUANT_SKN = 9,   /* GraphQuant over GraphSKNormal slices (GraphQSKNormalT, src/QAliases.jl:45-46): rrrmc_ctx_create_quant_skn per device */
    RRRMC_MODEL_QUANT_F64 = 10,  /* GraphQuant over sparse Float64 slices (GraphQEAT, src/QAliases.jl:50-83): rrrmc_ctx_create_quant_f64 per device */
    /* GraphRobustEnsemble (src/graphs/RE.jl:215-315) over GraphEmpty / binary GraphSK / GraphSKNormal slices: the model of a context made by
       rrrmc_ctx_create_re, and the selectors of rrrmc_ctx_create_multi for it (N = Nk, M; K ignored) */
    RRRMC_MODEL_RE_EMPTY = 11,   /* Graph0RE (src/REAliases.jl:20-29) */
    RRRMC_MODEL_RE_SK = 12,      /* GraphSKRE (src/REAliases.jl:33-38) */
    RRRMC_MODEL_RE_SKN = 13,     /* GraphRobustEnsemble(Nk, M, gamma, beta, GraphSKNormal, J) (test/runtests.jl:90-92) */
    /* GraphLocalEntropy (src/graphs/LE.jl:183-318) over GraphEmpty / binary GraphSK / GraphSKNormal slices: the model of a context made by
       rrrmc_ctx_create_le, and the selectors of rrrmc_ctx_create_multi for it (N = Nk, M; K ignored) */
    RRRMC_MODEL_LE_EMPTY = 14,   /* Graph0LE (src/LEAliases.jl:18-27) */
    RRRMC_MODEL_LE_SK = 15,      /* GraphSKLE (src/LEAliases.jl:31-38) */
    RRRMC_MODEL_LE_SKN = 16,     /* GraphLocalEntropy(Nk, M, gamma, beta, GraphSKNormal, J) (test/runtests.jl:103) */
    /* the binary perceptron trained on P random patterns (src/graphs/PercStep.jl, PercLinear.jl): the model of a context made by
       rrrmc_ctx_create_perc (N synapses; K and M ignored by rrrmc_ctx_create_multi) */
    RRRMC_MODEL_PERC_STEP = 17,    /* GraphPercStep(N, P): energy = the number of misclassified patterns (reported as Float64) */
    RRRMC_MODEL_PERC_LINEAR = 18,  /* GraphPercLinear(N, P) */
    /* the two ensembles over perceptron slices that share one pattern matrix (src/REAliases.jl, src/LEAliases.jl): made by
       rrrmc_ctx_create_re / _le with RRRMC_RE_SLICE_PERC_STEP / _PERC_LINEAR; selectors of rrrmc_ctx_create_multi (N = Nk, M; K ignored) */
    RRRMC_MODEL_RE_PERC_STEP = 19,   /* GraphPercStepRE */
    RRRMC_MODEL_RE_PERC_LINEAR = 20, /* GraphPercLinearRE */
    RRRMC_MODEL_LE_PERC_STEP = 21,   /* GraphPercStepLE */
    RRRMC_MODEL_LE_PERC_LINEAR = 22, /* GraphPercLinearLE */
    /* the two-layer binary committee machines (src/graphs/CommStep.jl, CommReLU.jl): made by rrrmc_ctx_create_comm; selectors of
       rrrmc_ctx_create_multi with N = K1*K2 and K = K2 (M ignored) */
    RRRMC_MODEL_COMM_STEP = 23,    /* GraphCommStep(K1, K2, P): energy = the number of misclassified patterns (reported as Float64) */
    RRRMC_MODEL_COMM_RELU = 24,    /* GraphCommReLU(K1, K2, P) */
    /* the two ensembles over committee machine slices that share one pattern matrix: made by rrrmc_ctx_create_re / _le with
       RRRMC_RE_SLICE_COMM_STEP / _COMM_RELU; selectors of rrrmc_ctx_create_multi (N = Nk, M; K ignored: rrrmc_set_comm_patterns fixes K2) */
    RRRMC_MODEL_RE_COMM_STEP = 25,   /* GraphCommStepRE */
    RRRMC_MODEL_RE_COMM_RELU = 26,   /* GraphCommReLURE */
    RRRMC_MODEL_LE_COMM_STEP = 27,   /* GraphCommStepLE */
    RRRMC_MODEL_LE_COMM_RELU = 28,   /* GraphCommReLULE */
    /* GraphQuant over pattern-machine slices that share one pattern matrix (src/QAliases.jl:85-159): selectors of rrrmc_ctx_create_multi only
       (N = Nk, K = K2 — ignored for the perceptrons —, M: rrrmc_ctx_create_quant_pattern per device; the contexts report RRRMC_MODEL_QUANT_RRG) */
    RRRMC_MODEL_QUANT_PERC_STEP = 29,   /* GraphQPercStepT */
    RRRMC_MODEL_QUANT_PERC_LINEAR = 30, /* GraphQPercLinearT */
    RRRMC_MODEL_QUANT_COMM_STEP = 31,   /* GraphQCommStepT */
    RRRMC_MODEL_QUANT_COMM_RELU = 32,   /* GraphQCommReLUT */
    /* random K-SAT (src/graphs/SAT.jl): the model of a context made by rrrmc_ctx_create_sat (N variables; K and M ignored by
       rrrmc_ctx_create_multi), and the two ensembles over SAT slices that share one clause set (src/REAliases.jl:77-92,
       src/LEAliases.jl:77-92): made by rrrmc_ctx_create_re / _le with RRRMC_RE_SLICE_SAT; selectors of rrrmc_ctx_create_multi (N = Nk, M) */
    RRRMC_MODEL_SAT = 33,      /* GraphSAT(N, K, alpha): energy = the number of violated clauses (reported as Float64) */
    RRRMC_MODEL_RE_SAT = 34,   /* GraphSATRE */
    RRRMC_MODEL_LE_SAT = 35,   /* GraphSATLE */
    /* the third committee machine (src/graphs/CommQu.jl): GraphCommQu by rrrmc_ctx_create_comm_qu, its ensembles by rrrmc_ctx_create_re / _le
       with RRRMC_RE_SLICE_COMM_QU, its GraphQuant by rrrmc_ctx_create_quant_pattern; selectors of rrrmc_ctx_create_multi as their siblings */
    RRRMC_MODEL_COMM_QU = 36,        /* GraphCommQu(K1, K2, P): energy = the number of misclassified patterns (reported as Float64) */
    RRRMC_MODEL_RE_COMM_QU = 37,     /* GraphCommQuRE */
    RRRMC_MODEL_LE_COMM_QU = 38,     /* GraphCommQuLE */
    RRRMC_MODEL_QUANT_COMM_QU = 39,  /* GraphQCommQuT (the contexts report RRRMC_MODEL_QUANT_RRG) */
    /* GraphTopologicalLocalEntropy (src/graphs/TLE.jl, src/TLEAliases.jl): the models of contexts made by rrrmc_ctx_create_tle, and the
       selectors of rrrmc_ctx_create_multi for it (N = Nk, M; K ignored).  40 .. 43 are unassigned. */
    RRRMC_MODEL_TLE_EMPTY = 44,  /* Graph0TLE */
    RRRMC_MODEL_TLE_SK = 45,     /* GraphSKTLE */
    RRRMC_MODEL_TLE_SKN = 46,    /* GraphTopologicalLocalEntropy(Nk, M, gamma, lambda, beta, GraphSKNormal, J) */
    RRRMC_MODEL_TLE_SAT = 47,    /* GraphSATTLE */
    /* GraphAddFields / GraphAddSubFields (src/graphs/AddFields.jl) over one graph g: the models of contexts made by rrrmc_ctx_create_af,
       and the selectors of rrrmc_ctx_create_multi for it (N; K = K2 for the committee machines, ignored otherwise; M ignored).
       48 + s for GraphAddFields and 57 + s for GraphAddSubFields, s numbering the nine kinds of g in the order of rrrmc_re_slice. */
    RRRMC_MODEL_AF_EMPTY = 48,        /* GraphAddFields(h, GraphEmpty(N)) */
    RRRMC_MODEL_AF_SK = 49,           /* GraphAddFields(h, GraphSK(J)) */
    RRRMC_MODEL_AF_SKN = 50,          /* GraphAddFields(h, GraphSKNormal(J)) */
    RRRMC_MODEL_AF_PERC_STEP = 51,    /* GraphAddFields(h, GraphPercStep) */
    RRRMC_MODEL_AF_PERC_LINEAR = 52,  /* GraphAddFields(h, GraphPercLinear) */
    RRRMC_MODEL_AF_COMM_STEP = 53,    /* GraphAddFields(h, GraphCommStep) */
    RRRMC_MODEL_AF_COMM_RELU = 54,    /* GraphAddFields(h, GraphCommReLU) */
    RRRMC_MODEL_AF_SAT = 55,          /* GraphAddFields(h, GraphSAT) */
    RRRMC_MODEL_AF_COMM_QU = 56,      /* GraphAddFields(h, GraphCommQu) */
    RRRMC_MODEL_ASF_EMPTY = 57,       /* GraphAddSubFields(h, GraphEmpty(N)) */
    RRRMC_MODEL_ASF_SK = 58,          /* GraphAddSubFields(h, GraphSK(J)) */
    RRRMC_MODEL_ASF_SKN = 59,         /* GraphAddSubFields(h, GraphSKNormal(J)) */
    RRRMC_MODEL_ASF_PERC_STEP = 60,   /* GraphAddSubFields(h, GraphPercStep) */
    RRRMC_MODEL_ASF_PERC_LINEAR = 61, /* GraphAddSubFields(h, GraphPercLinear) */
    RRRMC_MODEL_ASF_COMM_STEP = 62,   /* GraphAddSubFields(h, GraphCommStep) */
    RRRMC_MODEL_ASF_COMM_RELU = 63,   /* GraphAddSubFields(h, GraphCommReLU) */
    RRRMC_MODEL_ASF_SAT = 64,         /* GraphAddSubFields(h, GraphSAT) */
    RRRMC_MODEL_ASF_COMM_QU = 65,     /* GraphAddSubFields(h, GraphCommQu) */
    /* the cross-entropy perceptron (src/graphs/PercXEntr.jl): the model of a context made by rrrmc_ctx_create_perc_xentr (N synapses; K and
       M ignored by rrrmc_ctx_create_multi) */
    RRRMC_MODEL_PERC_XENTR = 66,      /* GraphPercXEntr(N, P, lambda) */
    /* the three ensembles over sparse Float64 slices (GraphEANormal: GraphEARE, GraphEALE, GraphEATLE of src/REAliases.jl:43-75,
       src/LEAliases.jl:43-75, src/TLEAliases.jl:36-68; GraphRRGNormal alike): made by rrrmc_ctx_create_re_f64 / _le_f64 / _tle_f64;
       selectors of rrrmc_ctx_create_multi (N = Nk, K, M) */
    RRRMC_MODEL_RE_SPARSE_F64 = 67,   /* GraphRobustEnsemble over (A, J) Float64 slices */
    RRRMC_MODEL_LE_SPARSE_F64 = 68,   /* GraphLocalEntropy over them */
    RRRMC_MODEL_TLE_SPARSE_F64 = 69,  /* GraphTopologicalLocalEntropy over them */
    /* the two field wrappers over GraphPercXEntr: made by rrrmc_ctx_create_af with RRRMC_RE_SLICE_PERC_XENTR; selectors of rrrmc_ctx_create_multi.
       70 .. 99 are unassigned: the wrappers' first eighteen ids are a closed block (48 .. 65), and so are their names */
    RRRMC_MODEL_XENTR_AF = 100,       /* GraphAddFields(h, GraphPercXEntr) */
    RRRMC_MODEL_XENTR_ASF = 101,      /* GraphAddSubFields(h, GraphPercXEntr) */
    /* GraphMixed (src/graphs/Mixed.jl) and the two field wrappers over it: the models of contexts made by rrrmc_ctx_create_mixed /
       rrrmc_ctx_create_mixed_multi (rrrmc_ctx_create_multi cannot carry a component list and refuses them) */
    RRRMC_MODEL_MIXED = 102,          /* GraphMixed(graphs...) */
    RRRMC_MODEL_MIXED_AF = 103,       /* GraphAddFields(h, GraphMixed(graphs...)) */
    RRRMC_MODEL_MIXED_ASF = 104,      /* GraphAddSubFields(h, GraphMixed(graphs...)) */
    /* the regular 3-spin model (src/graphs/PSpin3.jl) and the two field wrappers over it: the models of contexts made by
       rrrmc_ctx_create_pspin3; selectors of rrrmc_ctx_create_multi (N, K; M ignored) */
    RRRMC_MODEL_PSPIN3 = 105,         /* GraphPSpin3(N, K): energy = -(sum over the triples of the three spins' product) (reported as Float64) */
    RRRMC_MODEL_PSPIN3_AF = 106,      /* GraphAddFields(h, GraphPSpin3) */
    RRRMC_MODEL_PSPIN3_ASF = 107      /* GraphAddSubFields(h, GraphPSpin3) */
};

/* slice families of rrrmc_ctx_create_re */
enum rrrmc_re_slice {
    RRRMC_RE_SLICE_EMPTY = 0,    /* GraphEmpty (src/graphs/Empty.jl): zero residual, zero energy */
    RRRMC_RE_SLICE_SK = 1,       /* binary GraphSK (src/graphs/SK.jl:28-60): couplings with rrrmc_set_couplings_bits */
    RRRMC_RE_SLICE_SKN = 2,      /* GraphSKNormal (src/graphs/SK.jl:181-210): couplings with rrrmc_set_couplings_dense */
    RRRMC_RE_SLICE_PERC_STEP = 3,   /* GraphPercStep (src/graphs/PercStep.jl): patterns with rrrmc_set_patterns; Nk odd */
    RRRMC_RE_SLICE_PERC_LINEAR = 4, /* GraphPercLinear (src/graphs/PercLinear.jl): patterns with rrrmc_set_patterns; Nk odd */
    RRRMC_RE_SLICE_COMM_STEP = 5,   /* GraphCommStep (src/graphs/CommStep.jl): patterns with rrrmc_set_comm_patterns; Nk = K1*K2, K1, K2 odd */
    RRRMC_RE_SLICE_COMM_RELU = 6,   /* GraphCommReLU (src/graphs/CommReLU.jl): patterns and labels with rrrmc_set_comm_patterns; K1, K2 even */
    /* 7 is unassigned: rrrmc_ctx_create_re / _le refuse it with RRRMC_ERR_INVALID_ARG */
    RRRMC_RE_SLICE_SAT = 8,         /* GraphSAT (src/graphs/SAT.jl): clauses with rrrmc_set_clauses */
    RRRMC_RE_SLICE_COMM_QU = 9,     /* GraphCommQu (src/graphs/CommQu.jl): patterns and labels with rrrmc_set_comm_patterns; K1, K2 even */
    /* 10 is unassigned, like 7 */
    RRRMC_RE_SLICE_PERC_XENTR = 11, /* GraphPercXEntr (src/graphs/PercXEntr.jl): patterns with rrrmc_set_patterns, the table with rrrmc_set_loss_table;
                                       N odd.  The g of rrrmc_ctx_create_af only: rrrmc_ctx_create_re / _le / _tle / _quant_pattern refuse it
                                       (the reference has no RE, LE or Q alias for this graph) */
    RRRMC_RE_SLICE_SPARSE_F64 = 12, /* GraphEANormal / GraphRRGNormal (src/graphs/EA.jl:534-680, RRG.jl:503-617): (A, J) with rrrmc_set_graph_f64.
                                       The slice graph has a K of its own, so these contexts are made by rrrmc_ctx_create_re_f64 / _le_f64 /
                                       _tle_f64; rrrmc_ctx_create_re / _le / _tle refuse the kind and name that creator */
    RRRMC_RE_SLICE_MIXED = 13,      /* GraphMixed: the g of the field wrappers made by rrrmc_ctx_create_mixed only.  rrrmc_ctx_create_af, _re, _le,
                                       _tle and _quant_pattern refuse it, and so does a component list (a mix does not nest) */
    RRRMC_RE_SLICE_PSPIN3 = 14      /* GraphPSpin3 (src/graphs/PSpin3.jl): the g of the field wrappers made by rrrmc_ctx_create_pspin3 only.
                                       rrrmc_ctx_create_af, _re, _le, _tle, _quant_pattern and _mixed refuse it */
};

/* Library ABI version (major*10000 + minor*100 + patch). */
RRRMC_API int32_t rrrmc_version(void);

/* Text of the most recent error on this ctx (or of the last failed rrrmc_ctx_create when ctx == NULL).
 * The pointer stays valid until the next failing call on the same ctx / thread. */
RRRMC_API const char *rrrmc_last_error(const rrrmc_ctx *ctx);

/* Number of visible HIP devices (0 when there is none; never fails). */
RRRMC_API int32_t rrrmc_device_count(void);
/* Measurement helper (bench.py; SURVEY.md §8d "also report a measured device-copy bandwidth"): times `reps` device-to-device copies of
 * `nbytes` with HIP events on a private stream and returns (bytes read + bytes written) per second in GB/s. */
RRRMC_API int32_t rrrmc_device_copy_bandwidth(int32_t device, int64_t nbytes, int32_t reps, double *gbps_out);
/* Page-locked host memory for result buffers (optional).  Every entry point accepts ordinary host memory; a buffer from rrrmc_host_alloc
 * lets the copies of rrrmc_fetch_results / rrrmc_get_spins / rrrmc_standard_mc run at the bus rate instead of through the driver's
 * staging of pageable memory (the reference returns Es and C from every call, src/RRRMC.jl:126: at config 2 that is 64 MiB per call).
 * Free with rrrmc_host_free; both are independent of any context. */
RRRMC_API int32_t rrrmc_host_alloc(int64_t nbytes, void **out);
RRRMC_API int32_t rrrmc_host_free(void *p);

/*
 * Create a context for R replicas (chains) of one graph with N spins and K neighbour slots per spin.
 *   model     rrrmc_model
 *   device    HIP device ordinal
 *   replica0  global id of this ctx's first replica (replica ids address the random streams; a job of
 *             R_total replicas sharded over several devices passes the shard offset here; must be a
 *             multiple of 32)
 * Replaces: constructing the graph object + its LocalFields cache, src/graphs/RRG.jl:122-138.
 */
RRRMC_API int32_t rrrmc_ctx_create(rrrmc_ctx **out, int32_t model, int64_t N, int64_t K, int64_t R,
                                   int32_t device, uint32_t replica0);
/*
 * One context over SEVERAL devices (rrrmc_ctx_create(..., device_ids[], ndev)): what a reference user gets from one
 * standardMC call in one process (src/RRRMC.jl:81-88).  The R replicas are sharded over device_ids[0..ndev-1] in whole 32-replica
 * groups, in global-id order (a device may be named more than once: each entry gets its own shard and stream); replica ids address
 * the random streams, so every result is the one a single-device context gives.  Every function of this header that takes a ctx
 * accepts the multi-device context: per-replica buffers ([R], [R x nsamples], [R x chunks] ...) are the caller's full arrays and
 * arrive gathered; enqueueing calls return when every device has its work queued, rrrmc_sync / fetch / energy calls run one host
 * thread per device.  rrrmc_last_timing / rrrmc_timing_total report the slowest device.
 *   model  any rrrmc_model; RRRMC_MODEL_QUANT_RRG takes (N = Nk, K, M) as rrrmc_ctx_create_quant does, RRRMC_MODEL_QUANT_SK / _SKN take
 *          (N = Nk, M) as rrrmc_ctx_create_quant_sk / _skn do (K ignored), RRRMC_MODEL_QUANT_F64 takes (N = Nk, K, M) as rrrmc_ctx_create_quant_f64,
 *          RRRMC_MODEL_RE_EMPTY / _SK / _SKN take (N = Nk, M) as rrrmc_ctx_create_re does (K ignored), RRRMC_MODEL_LE_EMPTY / _SK / _SKN
 *          take (N = Nk, M) as rrrmc_ctx_create_le does (K ignored), and so do RRRMC_MODEL_RE_PERC_* / RRRMC_MODEL_LE_PERC_* and
 *          RRRMC_MODEL_RE_COMM_* / RRRMC_MODEL_LE_COMM_*; RRRMC_MODEL_COMM_STEP / _RELU / _QU take (N = K1*K2, K = K2) as rrrmc_ctx_create_comm / _comm_qu do;
 *          RRRMC_MODEL_PERC_STEP / _LINEAR take N as rrrmc_ctx_create_perc does; RRRMC_MODEL_AF_* / RRRMC_MODEL_ASF_* take (N, K = K2) as
 *          rrrmc_ctx_create_af does; M is ignored otherwise.
 */
RRRMC_API int32_t rrrmc_ctx_create_multi(rrrmc_ctx **out, int32_t model, int64_t N, int64_t K, int64_t M, int64_t R,
                                         const int32_t *device_ids, int32_t ndev, uint32_t replica0);
RRRMC_API void rrrmc_ctx_destroy(rrrmc_ctx *ctx);

/* Disorder: A[N*K] 0-based neighbours, J[N*K] couplings in {-1,+1}; J[x*K+k] belongs to the bond
 * (x, A[x*K+k]) and must be symmetric (checked).  Replaces GraphRRG{Int,(-1,1),K}(A, J), RRG.jl:122. */
RRRMC_API int32_t rrrmc_set_graph(rrrmc_ctx *ctx, const int32_t *A, const int8_t *J);

/* Random.seed!(seed) (src/RRRMC.jl:89): selects the Philox key and rewinds the iteration counter.
 * Not calling it between two sampling calls continues the streams (the reference's `seed <= 0`). */
RRRMC_API int32_t rrrmc_seed(rrrmc_ctx *ctx, uint64_t seed);

/* Config(N) with random spins for every replica (src/Interface.jl:24-28), INIT stream of the seed. */
RRRMC_API int32_t rrrmc_init_spins_random(rrrmc_ctx *ctx);
/* C0 (src/RRRMC.jl:93): chunks[R * ceil(N/64)] in BitVector layout. */
RRRMC_API int32_t rrrmc_set_spins(rrrmc_ctx *ctx, const uint64_t *chunks);
RRRMC_API int32_t rrrmc_get_spins(rrrmc_ctx *ctx, uint64_t *chunks);

/* energy(X, C) for every replica (src/Interface.jl:105, src/graphs/RRG.jl:164-189): E_out[R] (int64).
 * Also rebuilds the device-side caches, exactly as the reference's `energy` resets LocalFields. */
RRRMC_API int32_t rrrmc_energy(rrrmc_ctx *ctx, int64_t *E_out);

/* Debug/parity view of the cache: lfields_out[R * N] (int64), lfields[x] = -delta_energy(X, C, x)
 * (src/graphs/RRG.jl:236-244), recomputed from the current spins. */
RRRMC_API int32_t rrrmc_get_fields(rrrmc_ctx *ctx, int64_t *lfields_out);

/*
 * standardMC(X, beta, iters; step) for all R replicas (src/RRRMC.jl:81-127).
 *   Es_out        [R * (iters / step)] int64, replica-major: the energy BEFORE the move of iteration
 *                 k*step (src/RRRMC.jl:104-108).  May be NULL.
 *   accepted_out  [R] accepted moves of this call.  May be NULL.
 * The configuration is resumed from the ctx and left updated (C0 is mutated in place, RRRMC.jl:93).
 * Synchronous: returns when the results are on the host.
 * beta: any value but NaN (RRRMC_ERR_INVALID_ARG), as in the reference — except on RRRMC_MODEL_SPARSE_PM1, whose kernels (and
 * rrrmc_colored_sweeps*) accept every move with dE <= 0 unconditionally: beta < 0, and an infinite beta on a graph of even degree (a move
 * with dE = 0 has x = NaN there, rejected by the reference), are refused with RRRMC_ERR_UNSUPPORTED.
 */
RRRMC_API int32_t rrrmc_standard_mc(rrrmc_ctx *ctx, double beta, int64_t iters, int64_t step,
                                    int64_t *Es_out, int64_t *accepted_out);

/* Device-resident form of the same call: enqueue on the ctx's stream and return; results stay in HBM
 * until fetched.  rrrmc_sync waits for the stream.  Used by bench.py for the timed region. */
RRRMC_API int32_t rrrmc_standard_mc_async(rrrmc_ctx *ctx, double beta, int64_t iters, int64_t step);
RRRMC_API int32_t rrrmc_sync(rrrmc_ctx *ctx);
/* Results of the last (a)sync sampling call: Es_out[R * nsamples] replica-major, accepted_out[R]. */
RRRMC_API int32_t rrrmc_fetch_results(rrrmc_ctx *ctx, int64_t *Es_out, int64_t *accepted_out);
/* The build of the LDS-resident sweep kernel the last standardMC call on a sparse +-J context launched: -1 = none yet (or the call took
 * another kernel: graphs beyond LDS), 0 = the generic kernel, else the zero-block pattern the build is specialised for, two bits per
 * class of dE > 0, class 0 lowest: the number of leading four-plane blocks of that class's acceptance threshold the build takes as
 * zero (beta = 1 at K = 3: 2 = two blocks of class 0, none of class 1).  RRRMC_SWEEP_GENERIC=1 in the environment of a call selects the
 * generic kernel.  Multi-device contexts report their first shard. */
RRRMC_API int32_t rrrmc_sweep_build(rrrmc_ctx *ctx, int32_t *build_out);
/* Which kernels the last standardMC or colour-sweep call on a sparse +-J context launched, and the layout they ran in (out: four values):
 *   out[0]  the path: 0..3 = sweep_kernel MODE 0..3 (0 neighbour table in LDS, 1 table in HBM / byte offsets, 2 table in HBM / word
 *           indices, 3 one word per site); 4 = big_mask_kernel + big_apply_kernel; 5 = big_mask_kernel + big_applyc_kernel (compact
 *           masks); 6 = big_sweep_kernel (no mask pass); 7 = colour sweep, plain build; 8 = colour sweep, the build that counts accepted
 *           moves; -1 = no such call yet
 *   out[1]  K
 *   out[2]  the chunk length C of the context
 *   out[3]  lg2 of the replicas per workgroup of the big-N path (paths 4..6), else -1
 * The layout is chosen at context creation; tests move it with RRRMC_FORCE_WIDE (1: table in HBM; 2: word indices, MODE 2, at any
 * N <= 32767), RRRMC_FORCE_SINGLE, RRRMC_FORCE_BIG, RRRMC_BIG_NO_MASKS and RRRMC_BIG_LGR (0..5: 2^n replicas per workgroup, honoured where
 * n is no larger than the size's own value).  Multi-device contexts report their first shard. */
RRRMC_API int32_t rrrmc_sweep_layout(rrrmc_ctx *ctx, int32_t *out);

/* ---- colour-parallel ("checkerboard") sweeps: build-defined extension for large sparse graphs ---------------------
 * The reference's standardMC is random-site (src/RRRMC.jl:113) and its kernel here keeps a replica group's spins in
 * LDS (one or two 4-byte words per site next to the chunk buffers: up to N = 32 767).  For larger graphs (BASELINE.json
 * config 4: GraphEA L=64, D=3) the engine offers sweeps over a
 * proper colouring: one sweep attempts every site once, colour by colour, all sites of a colour at once, with the
 * reference's delta_energy and accept rule (src/graphs/EA.jl:266-275, src/RRRMC.jl:39).  A ctx of
 * RRRMC_MODEL_SPARSE_PM1 whose state does not fit the LDS sweep still runs rrrmc_standard_mc* (random-site, the same chain, through
 * the big-N kernels: N <= 2^20, roughly ten times slower than these sweeps).
 *   color[N] in 0..ncolors-1, adjacent sites must differ (checked).  Call after rrrmc_set_graph: the colouring is stored as per-site
 *   records of that graph, and a later rrrmc_set_graph drops it (rrrmc_colored_sweeps_async then returns RRRMC_ERR_STATE).
 *   rrrmc_colored_sweeps_async: `sweeps` sweeps; an energy sample is taken BEFORE sweep k*step (as RRRMC.jl:104-108
 *   with a sweep as the unit); results through rrrmc_sync + rrrmc_fetch_results (Es [R x sweeps/step]; accepted_out
 *   is not tracked by this sampler and reads -1). */
RRRMC_API int32_t rrrmc_set_coloring(rrrmc_ctx *ctx, const int32_t *color, int32_t ncolors);
RRRMC_API int32_t rrrmc_colored_sweeps_async(rrrmc_ctx *ctx, double beta, int64_t sweeps, int64_t step);
/* on != 0: the colour sweeps also count every replica's accepted moves (fetched like standardMC's accepted counts; a few per cent
 * slower: one 32x32 bit transpose per wavefront and site).  Default off: accepted_out reads -1 after a colour-sweep call. */
RRRMC_API int32_t rrrmc_colored_count_accepted(rrrmc_ctx *ctx, int32_t on);

/* ---- Float64-energy models (RRRMC_MODEL_SK_NORMAL): ET = Float64 (src/graphs/SK.jl:181) --------------------
 * Dense couplings J[N*N] row-major; must be symmetric with a zero diagonal (GraphSKNormal(J; check=true),
 * SK.jl:184-195: violations are RRRMC_ERR_INVALID_ARG).  Replaces GraphSKNormal(J). */
RRRMC_API int32_t rrrmc_set_couplings_dense(rrrmc_ctx *ctx, const double *J);
/* energy / cache / sampler results as Float64 (same meaning as the integer forms above; delta_energy = +lfields,
 * SK.jl:278-284).  rrrmc_standard_mc_async / rrrmc_sync are shared by all models. */
RRRMC_API int32_t rrrmc_energy_f64(rrrmc_ctx *ctx, double *E_out);
RRRMC_API int32_t rrrmc_get_fields_f64(rrrmc_ctx *ctx, double *lfields_out);
RRRMC_API int32_t rrrmc_standard_mc_f64(rrrmc_ctx *ctx, double beta, int64_t iters, int64_t step,
                                        double *Es_out, int64_t *accepted_out);
RRRMC_API int32_t rrrmc_fetch_results_f64(rrrmc_ctx *ctx, double *Es_out, int64_t *accepted_out);
/* RRRMC_MODEL_SK_BINARY: couplings as N BitVector rows of ceil(N/64) chunks (GraphSK(J::Vector{BitVector}), SK.jl:34-48):
 * symmetric, zero diagonal (checked).  The integer cache is read with rrrmc_get_fields (lfields = sqrt(N) * delta_energy,
 * SK.jl:137-140), energies with the _f64 entry points.  rrrmc_gen_sk_binary = gen_J (SK.jl:17-26), SKBITS stream. */
RRRMC_API int32_t rrrmc_set_couplings_bits(rrrmc_ctx *ctx, const uint64_t *J_chunks);
RRRMC_API int32_t rrrmc_gen_sk_binary(int64_t N, uint64_t seed, uint64_t *J_chunks_out);
/* gen_J_gauss (src/graphs/SK.jl:170-179): J_out[N*N], normal(0, 1/N), symmetric, zero diagonal. GAUSS stream. */
RRRMC_API int32_t rrrmc_gen_sk_gauss(int64_t N, uint64_t seed, double *J_out);

/* ---- GraphQuant + rrrMC (RRRMC_MODEL_QUANT_RRG) ---------------------------------------------------------------
 * N = Nk * M spins per replica, slice-major (slice k holds spins k*Nk .. (k+1)*Nk-1, QT.jl:105-108); the slice graph's
 * (A, J) [Nk x K] is given with rrrmc_set_graph.  Energies are Float64: use the _f64 entry points for energy / results.
 * Replaces GraphQuant{fourK,GraphRRG}(...) (QT.jl:139-170).  The slice graph must be simple (no repeated bonds: a GraphEA with L = 2 is
 * refused).  rrrmc_bkl_mc_async / rrrmc_wtm_mc_async run the generic continuous-energy caches over all Nk * M spins (DeltaE.jl:315) with
 * neighbors(X, i) = the two Trotter neighbours, then the slice graph's (QT.jl:288-321); rrrmc_quant_set_field must have been called. */
RRRMC_API int32_t rrrmc_ctx_create_quant(rrrmc_ctx **out, int64_t Nk, int64_t K, int64_t M, int64_t R,
                                         int32_t device, uint32_t replica0);
/* GraphQuant over binary GraphSK slices — GraphQSKT(Nk, M, Gamma, beta) = GraphQuant(Nk, M, Gamma, beta, GraphSK, gen_J(Nk))
 * (src/QAliases.jl:34-43), the graph of the reference's quantum experiment (scripts/scripts.jl:766-864, test_QIsing).  The slice
 * couplings are given with rrrmc_set_couplings_bits (Nk rows of ceil(Nk/64) chunks, as for RRRMC_MODEL_SK_BINARY; rrrmc_gen_sk_binary
 * draws them); everything else is as for rrrmc_ctx_create_quant: rrrmc_quant_set_field, rrrmc_rrr_mc_async, rrrmc_standard_mc_async,
 * rrrmc_energy_f64, rrrmc_quant_observables.  delta_energy_residual = (lfields[i] / sqrt(Nk)) / M (SK.jl:137-140, QT.jl:270-281) with
 * the integer field recomputed by popcounts of the slice's spin words against row i of J. */
RRRMC_API int32_t rrrmc_ctx_create_quant_sk(rrrmc_ctx **out, int64_t Nk, int64_t M, int64_t R, int32_t device, uint32_t replica0);
/* GraphQuant over M GraphSKNormal slices sharing one Gaussian coupling matrix (GraphQSKNormalT, src/QAliases.jl:45-46 — one of the graphs
 * of the reference's own test loop, test/runtests.jl:80): then rrrmc_set_couplings_dense(ctx, J[Nk x Nk]) and rrrmc_quant_set_field.
 * rrrMC (rrrmc_rrr_mc_async) and standardMC are wired (thread per replica, every slice keeps its Float64 lfields / lfields_last / move_last
 * exactly as SK.jl:212-276 updates them); bklMC / wtmMC / extremal_opt and the observables are not (RRRMC_ERR_UNSUPPORTED). */
RRRMC_API int32_t rrrmc_ctx_create_quant_skn(rrrmc_ctx **out, int64_t Nk, int64_t M, int64_t R, int32_t device, uint32_t replica0);
/* GraphQuant over M sparse Float64 slices sharing one (A, J::Float64) — GraphQEAT = GraphQuant{fourK,GraphEANormal{twoD}}
 * (src/QAliases.jl:50-83: GraphQEAT(L, D, M, Gamma, beta), GraphQEAT(fname, M, Gamma, beta), GraphQEAT(X::GraphEANormal, M, Gamma, beta)), and the
 * same over a GraphRRGNormal: then rrrmc_set_graph_f64(ctx, A[Nk x K], J[Nk x K]) (sorted rows, symmetric; a neighbour may repeat: L = 2) and
 * rrrmc_quant_set_field.  Every slice keeps its own LocalFields{Float64}: lfields, the live part of lfields_last (the K + 1 values the undo
 * path of update_cache! reads, src/graphs/EA.jl:613-653 / RRG.jl:576-617) and move_last, per replica.  K <= 8.  Samplers: rrrmc_rrr_mc_async
 * (rrrMC(X::DoubleGraph), src/RRRMC.jl:221-290: delta_energy_residual = -lfields[i] / M, src/graphs/QT.jl:270-281), rrrmc_standard_mc_async, and
 * the generic caches over all Nk * M spins — rrrmc_bkl_mc_async, rrrmc_wtm_mc_async, rrrmc_extremal_opt_async (neighbors = the two Trotter
 * neighbours, then the slice graph's, QT.jl:288-321); one thread per replica.  rrrmc_quant_observables is not wired for these slices. */
RRRMC_API int32_t rrrmc_ctx_create_quant_f64(rrrmc_ctx **out, int64_t Nk, int64_t K, int64_t M, int64_t R, int32_t device, uint32_t replica0);
/* GraphQuant over M pattern machines that share one pattern matrix — GraphQPercStepT, GraphQPercLinearT, GraphQCommStepT, GraphQCommReLUT,
 * GraphQCommQuT (src/QAliases.jl:85-181).  slice_kind is RRRMC_RE_SLICE_PERC_STEP / _PERC_LINEAR / _COMM_STEP / _COMM_RELU / _COMM_QU; Nk synapses
 * per slice, for the committee machines Nk = K1*K2 (K2 is ignored for the perceptrons).  RRRMC_ERR_INVALID_ARG: Nk even (perceptrons); K1, K2 even
 * (step) or odd (ReLU, Qu), Nk not a multiple of K2; M <= 2 (QT.jl:47).  RRRMC_ERR_UNSUPPORTED: Nk > 32767, N = Nk*M > 65535.  Then rrrmc_set_patterns
 * (perceptrons) or rrrmc_set_comm_patterns (committee machines; 1 <= P <= 4096) and rrrmc_quant_set_field, without which every sampler,
 * energy and observable call answers RRRMC_ERR_STATE.  Sites are GraphQuant's, x = k*Nk + i.  energy = energy(GraphQT) + sum_k
 * energy(X1[k]) / M (QT.jl:185-199); delta_energy_residual = delta_energy(X1[k], C1[k], i) / M (QT.jl:270-281).  Served by rrrmc_rrr_mc_async
 * (rrrMC(X::DoubleGraph), the DeltaECache over GraphQT only), rrrmc_standard_mc_async, rrrmc_energy_f64, rrrmc_set_resume,
 * rrrmc_set_debug_checks (Stabilities, masks and E recomputed after a call), rrrmc_rrr_cache, the spin / snapshot / overlap calls,
 * rrrmc_quant_observables and rrrmc_quant_renergies; one wavefront or one thread per replica (rrrmc_quant_pattern_build).  rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and
 * rrrmc_extremal_opt_async answer RRRMC_ERR_UNSUPPORTED (DeltaECacheCont over AllButOne neighbourhoods, as on the stand-alone graphs). */
RRRMC_API int32_t rrrmc_ctx_create_quant_pattern(rrrmc_ctx **out, int32_t slice_kind, int64_t Nk, int64_t K2, int64_t M, int64_t R,
                                                 int32_t device, uint32_t replica0);
/* The Trotter coupling fourK (a type parameter of GraphQuant in the reference, QT.jl:126) and the beta it was derived
 * from: needed by rrrmc_energy_f64 before the first rrrMC call, and by rrrmc_standard_mc_async — standardMC on the GraphQuant
 * (src/RRRMC.jl:81-127 with delta_energy = delta_energy(X0) + delta_energy_residual, QT.jl:283-286; SITE + ACCEPT_F64 streams),
 * which takes fourK from here. */
/* GraphQuant over GraphEA slices (ea_form = 1; call before rrrmc_set_graph): the slice graph may list a neighbour twice (L = 2: two bonds
 * to the same site) — delta_energy sums every entry, neighbors() of the continuous-energy caches is the de-duplicated list (EA.jl:158). */
RRRMC_API int32_t rrrmc_quant_slice_form(rrrmc_ctx *ctx, int32_t ea_form);
RRRMC_API int32_t rrrmc_quant_set_field(rrrmc_ctx *ctx, double beta, double fourK);
/* ---- GraphRobustEnsemble (src/graphs/RE.jl; RRRMC_MODEL_RE_*) -----------------------------------------------------
 * The Robust Ensemble of M replicas of one graph: the inner graph GraphRE{M,gamma,beta} couples the M replicas of every spin i through
 * mu_i = sum_k sigma_(i,k) (energy sum_i -log(2 cosh(gamma mu_i)) / beta), and replica k is slice k of a DoubleGraph whose residual is the slice
 * graph's delta_energy (NOT divided by M, RE.jl:303-310).  All M slices share one coupling set (Gconstr(args...) with the same args).
 *   N = Nk * M spins per replica of the batch, in the reference's site order: site j (0-based) is spin i = j / M of ensemble replica
 *   k = j % M (RE.jl:76-95) — in every configuration that crosses this ABI (rrrmc_set_spins / rrrmc_get_spins / rrrmc_init_spins_random, whose
 *   INIT stream is indexed by j) and in rrrmc_rrr_cache (the class of site j; the ArraySets hold site ids in the reference's member order).
 *   3 <= M <= 32, N <= 65 535.  Energies are Float64 (_f64 entry points).
 * rrrmc_ctx_create_re: slice_kind rrrmc_re_slice; then the couplings (rrrmc_set_couplings_bits [Nk rows] for _SK, rrrmc_set_couplings_dense
 * [Nk x Nk] for _SKN, nothing for _EMPTY) and rrrmc_re_set_params.  Samplers: rrrmc_rrr_mc_async (rrrMC(X::DoubleGraph), src/RRRMC.jl:221-290:
 * the DeltaECache over L = ceil(M/2) levels; fourK is ignored; streams as GraphQuant's) and rrrmc_standard_mc_async /
 * rrrmc_standard_mc_f64 (standardMC, SITE + ACCEPT_F64 streams); with the resume, debug-check, timing, results and cache entry points of the
 * other models.  rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and rrrmc_extremal_opt_async return RRRMC_ERR_UNSUPPORTED. */
RRRMC_API int32_t rrrmc_ctx_create_re(rrrmc_ctx **out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0);
/* The type parameters gamma and beta of GraphRE{M,gamma,beta} (beta_graph: the beta inside fk and the mu-energies, not the sampler's): builds the level table
 * and the mu-energy table on the host (rrrmc_re_tables).  Required before the first sampler or energy call; a change ends a resumed run. */
RRRMC_API int32_t rrrmc_re_set_params(rrrmc_ctx *ctx, double gamma, double beta_graph);
/* REenergies(X) (RE.jl:285-301): out[R * M], energy(X1[k], C1[k]) of every slice of every replica for the current configuration, in the
 * reference's summation order (SK.jl:62-96, 212-237).  Reads the configuration only — unlike the reference's, it does not rebuild the slice
 * caches, so a hook that calls it leaves the run as it was. */
RRRMC_API int32_t rrrmc_re_energies(rrrmc_ctx *ctx, double *out);
/* Host-only (no device needed): dElist[M] = DeltaElist(GraphRE{M,gamma,beta}) = fk(mu) for mu = -(M-1), -(M-3), ..., M-1 (RE.jl:18-26, 53-56; the
 * upper ceil(M/2) entries are allDeltaE), e0[M+1] = log(2 cosh(gamma mu)) / beta for mu = -M, -M+2, ..., M (RE.jl:90-93), evaluated with libm. */
RRRMC_API int32_t rrrmc_re_tables(int64_t M, double gamma, double beta, double *dElist, double *e0);

/* ---- The binary perceptron (src/graphs/PercStep.jl, PercLinear.jl; RRRMC_MODEL_PERC_*, RRRMC_RE_SLICE_PERC_*) ------
 * rrrmc_ctx_create_perc: R chains of GraphPercStep (linear = 0) or GraphPercLinear (linear != 0) with N synapses.  N must be odd
 * (RRRMC_ERR_INVALID_ARG, as the reference's ArgumentError) and at most 32767 (RRRMC_ERR_UNSUPPORTED: 16-bit stabilities).  Spins: one
 * bit per synapse in 64-bit chunks, as every chunk-layout model.  Then rrrmc_set_patterns.  Sampler: rrrmc_standard_mc_async
 * (src/RRRMC.jl:81-127) with rrrmc_fetch_results_f64 (GraphPercStep's integer energies arrive as exact Float64s), rrrmc_set_resume,
 * rrrmc_set_debug_checks, rrrmc_energy_f64.  rrrMC / bklMC / wtmMC / extremal_opt answer RRRMC_ERR_UNSUPPORTED: on these graphs they go
 * through DeltaECacheCont with AllButOne neighbourhoods, which is not wired.
 *
 * rrrmc_set_patterns: the P patterns xi[P * ceil(N / 64)], row a = pattern a as ceil(N / 64) chunks, bit i of a row = xi[a, i] (the xi_v
 * layout of gen_xi, PercStep.jl:19-29); bits beyond N must be 0.  1 <= P <= 4096 (RRRMC_ERR_UNSUPPORTED beyond).  For a context made by
 * rrrmc_ctx_create_perc, or by rrrmc_ctx_create_re / _le with a perceptron slice kind (N = Nk: all slices, and the centre of a
 * GraphLocalEntropy, share the one matrix).  May be called again: a new matrix (or a new P) ends a resumed run. */
RRRMC_API int32_t rrrmc_ctx_create_perc(rrrmc_ctx **out, int64_t N, int32_t linear, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_set_patterns(rrrmc_ctx *ctx, const uint64_t *xi, int64_t P);
/* gen_xi (PercStep.jl:19-29; the reference's bitrand is unpinned): xi_out[P * ceil(N / 64)] in the layout of rrrmc_set_patterns, drawn on
 * the host from the SKBITS stream of `seed` (third counter word 1).  Needs no device. */
RRRMC_API int32_t rrrmc_gen_patterns(int64_t N, int64_t P, uint64_t seed, uint64_t *xi_out);

/* ---- The cross-entropy perceptron (src/graphs/PercXEntr.jl; RRRMC_MODEL_PERC_XENTR, RRRMC_RE_SLICE_PERC_XENTR) ------
 * rrrmc_ctx_create_perc_xentr: R chains of GraphPercXEntr with N synapses; the argument checks of rrrmc_ctx_create_perc (N odd, N <= 32767).
 * Then rrrmc_set_patterns (1 <= P <= 4096) and rrrmc_set_loss_table, in either order; a sampling or energy call before both is
 * RRRMC_ERR_STATE.  energy = sum_a Hs[(Delta_a + N) / 2] and delta_energy = sum_a (Hs[new] - Hs[old]), both added in pattern order from 0.0
 * as PercXEntr.jl:97-119 and :165-193 add them: Float64 trajectories equal the reference's bit for bit GIVEN THE SAME TABLE.  Sampler:
 * rrrmc_standard_mc_async with rrrmc_fetch_results_f64, rrrmc_set_resume, rrrmc_set_debug_checks, rrrmc_energy_f64.  rrrMC / bklMC / wtmMC
 * / extremal_opt answer RRRMC_ERR_UNSUPPORTED as on the other stand-alone perceptrons; rrrMC runs on GraphAddFields / GraphAddSubFields over
 * it (rrrmc_ctx_create_af with RRRMC_RE_SLICE_PERC_XENTR).
 *
 * rrrmc_set_loss_table: Hs[n], n = N + 1, Hs[k] = log(1 + exp(-2 lambda Delta / sqrt(N))) for Delta = -N + 2 k (PercXEntr.jl:65), made by the
 * caller (a Julia caller passes X.Hs itself: Julia's log / exp and this library's libm do not promise the same last bit).  Every entry
 * must be finite (RRRMC_ERR_INVALID_ARG; the reference would carry Inf - Inf into accept).  For a context made by
 * rrrmc_ctx_create_perc_xentr or by rrrmc_ctx_create_af over it, single or multi-device.  May be called again (GraphPercXEntr(X, lambda_new):
 * annealing lambda on fixed patterns): a new table ends a resumed run, the next call starts from energy(X, C).
 *
 * rrrmc_xentr_build: the kernel build of the last standardMC call on a stand-alone GraphPercXEntr: 0 none yet, 1 one thread per chain, 2 one
 * wavefront per chain (few chains).  RRRMC_XENTR_NO_WAVE=1 forces 1, RRRMC_XENTR_WAVE=1 forces 2; RRRMC_XENTR_NO_LDS=1 keeps the table in
 * global memory in either.  All builds give the same bits.
 *
 * rrrmc_perc_step_energy: step_energy (PercXEntr.jl:205-213) of every chain's live configuration, out[R]: the number of patterns with
 * Delta_a < 0 (the training error), computed on the device from the configuration.  Read-only: a resumed run is not disturbed.  For any
 * stand-alone perceptron context and for rrrmc_ctx_create_af over a perceptron. */
RRRMC_API int32_t rrrmc_ctx_create_perc_xentr(rrrmc_ctx **out, int64_t N, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_set_loss_table(rrrmc_ctx *ctx, const double *Hs, int64_t n);
RRRMC_API int32_t rrrmc_xentr_build(rrrmc_ctx *ctx, int32_t *build_out);
RRRMC_API int32_t rrrmc_perc_step_energy(rrrmc_ctx *ctx, int64_t *out);

/* ---- The binary committee machines (src/graphs/CommStep.jl, CommReLU.jl; RRRMC_MODEL_COMM_*, RRRMC_RE_SLICE_COMM_*) ------
 * rrrmc_ctx_create_comm: R chains of GraphCommStep (relu = 0; K1 and K2 odd) or GraphCommReLU (relu != 0; K1 and K2 even) with K2 hidden
 * units of K1 synapses each, N = K1*K2 (unit k owns synapses k*K1 .. (k+1)*K1 - 1).  A wrong parity is RRRMC_ERR_INVALID_ARG (the
 * reference's ArgumentError), N > 32767 RRRMC_ERR_UNSUPPORTED (16-bit stabilities).  Spins: one bit per synapse in 64-bit chunks.  Then
 * rrrmc_set_comm_patterns.  Sampler: rrrmc_standard_mc_async with rrrmc_fetch_results_f64 (integer energies as exact Float64s),
 * rrrmc_set_resume, rrrmc_set_debug_checks, rrrmc_energy_f64.  rrrMC / bklMC / wtmMC / extremal_opt answer RRRMC_ERR_UNSUPPORTED.
 *
 * rrrmc_set_comm_patterns: the P patterns xi[P * ceil(N / 64)] in rrrmc_set_patterns' layout (bits beyond N must be 0), and for
 * GraphCommReLU and GraphCommQu the labels y[ceil(P / 64)] (bit a = y_a; bits beyond P must be 0); y must be NULL for GraphCommStep.  1 <= P <= 4096
 * (RRRMC_ERR_UNSUPPORTED beyond).  N % K2 != 0, a wrong parity of K1 = N / K2 or K2, a missing or extra y: RRRMC_ERR_INVALID_ARG.  For a
 * context made by rrrmc_ctx_create_comm (K2 must be the context's), or by rrrmc_ctx_create_re / _le with a committee slice kind (N = Nk:
 * this call fixes K2; all slices, and the centre of a GraphLocalEntropy, share the one matrix).  May be called again: it ends a resumed run. */
RRRMC_API int32_t rrrmc_ctx_create_comm(rrrmc_ctx **out, int64_t K1, int64_t K2, int32_t relu, int64_t R, int32_t device, uint32_t replica0);
/* GraphCommQu (src/graphs/CommQu.jl; RRRMC_MODEL_COMM_QU, RRRMC_RE_SLICE_COMM_QU): the committee machine whose hidden units answer with the
 * square of their stability, Delta2[a] = o_a sum_u c_u Delta1[u][a]^2, energy = #{Delta2 <= 0}.  K1 and K2 even, labels required: everything
 * said of GraphCommReLU above holds (rrrmc_set_comm_patterns with y, rrrmc_gen_comm_patterns, the samplers served and refused, N <= 32767);
 * the reference's per-pattern heaps are not kept, Delta2 is 32-bit. */
RRRMC_API int32_t rrrmc_ctx_create_comm_qu(rrrmc_ctx **out, int64_t K1, int64_t K2, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_set_comm_patterns(rrrmc_ctx *ctx, int64_t K2, const uint64_t *xi, const uint64_t *y, int64_t P);
/* gen_xi (CommStep.jl:16-26, CommReLU.jl:16-27, fc: CommStep.jl:85-93), drawn on the host: xi_out[P * ceil(K1*K2 / 64)] as
 * rrrmc_gen_patterns(fc ? K1 : K1*K2, P, seed) draws its rows, with fc's K1 columns repeated K2 times; y_out[ceil(P / 64)] (may be NULL)
 * from the SKBITS stream of `seed` with third counter word 2.  Needs no device. */
RRRMC_API int32_t rrrmc_gen_comm_patterns(int64_t K1, int64_t K2, int64_t P, int32_t fc, uint64_t seed, uint64_t *xi_out, uint64_t *y_out);

/* ---- Random K-SAT (src/graphs/SAT.jl; RRRMC_MODEL_SAT, RRRMC_MODEL_RE_SAT, RRRMC_MODEL_LE_SAT, RRRMC_RE_SLICE_SAT) ------
 * rrrmc_ctx_create_sat: R chains of GraphSAT with N variables, N <= 65535 (RRRMC_ERR_UNSUPPORTED beyond: 16-bit variable ids).  Spins: one
 * bit per variable in 64-bit chunks, as every chunk-layout model.  Then rrrmc_set_clauses.  Sampler: rrrmc_standard_mc_async
 * (src/RRRMC.jl:81-127) with rrrmc_fetch_results_f64 (the integer energies arrive as exact Float64s), rrrmc_set_resume,
 * rrrmc_set_debug_checks, rrrmc_energy_f64.  delta_energy is recomputed from the spins: there is no cache to keep.  rrrMC / bklMC / wtmMC /
 * extremal_opt answer RRRMC_ERR_UNSUPPORTED on the stand-alone graph (an integer DeltaECache of max_conn + 1 levels over variable-degree
 * neighbourhoods is not wired); rrrMC runs on the two ensembles.
 *
 * rrrmc_set_clauses: Mc clauses as vars[Mc * Kmax] (0-based variables in ascending order, short clauses padded with -1 at the end) and
 * lits[Mc * Kmax] (literal k of clause a is satisfied iff spin vars[a][k] == lits[a][k]; pads ignored).  RRRMC_ERR_INVALID_ARG: an empty
 * clause, a variable out of range, a variable twice in one clause, variables not ascending, a literal bit above 1.  RRRMC_ERR_UNSUPPORTED:
 * a clause of more than 8 literals, Mc > 2^20, a variable in more than 65535 clauses.  For a context made by rrrmc_ctx_create_sat, or by
 * rrrmc_ctx_create_re / _le with RRRMC_RE_SLICE_SAT (N = Nk: all slices, and the centre of a GraphLocalEntropy, share the one clause
 * set).  May be called again: it ends a resumed run.
 *
 * rrrmc_sat_build: the kernel build of the last standardMC call on a stand-alone GraphSAT: 0 none yet, 1 one thread per replica
 * (R > 16384, or RRRMC_SAT_NO_WAVE=1), 2 one wavefront per replica (R <= 16384: the two cross between 16384 and 32768 replicas, profiles/r12/sat.md; or RRRMC_SAT_WAVE=1).
 * Both give the same bits. */
RRRMC_API int32_t rrrmc_ctx_create_sat(rrrmc_ctx **out, int64_t N, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_set_clauses(rrrmc_ctx *ctx, int64_t Mc, int64_t Kmax, const int32_t *vars, const int8_t *lits);
RRRMC_API int32_t rrrmc_sat_build(rrrmc_ctx *ctx, int32_t *build_out);
/* The checks of rrrmc_set_clauses on the host alone, for N variables: the same codes and messages (a context-free failure: the text is
 * rrrmc_last_error(NULL)); max_conn_out (may be NULL) receives max |T[i]|.  Needs no device. */
RRRMC_API int32_t rrrmc_check_clauses(int64_t N, int64_t Mc, int64_t Kmax, const int32_t *vars, const int8_t *lits, int64_t *max_conn_out);
/* gen_randomKSAT / choose (SAT.jl:17-56; the reference's rand is unpinned): Mc = round(alpha * N) (ties to even) clauses of K distinct
 * ascending variables, vars_out[Mc * K] and lits_out[Mc * K] in the layout of rrrmc_set_clauses.  Draw n = a*K + k: the variable is
 * 1 + floor(u64(GRAPH, n) * (N - k) / 2^64) followed by choose's bump and sorted insert; the literal bit of sorted position k is the top
 * bit of u64(COUPLING, n).  Both arrays NULL: only Mc_out is written.  Needs no device. */
RRRMC_API int32_t rrrmc_gen_ksat(int64_t N, int64_t K, double alpha, uint64_t seed, int64_t *Mc_out, int32_t *vars_out, int8_t *lits_out);

/* ---- GraphLocalEntropy (src/graphs/LE.jl; RRRMC_MODEL_LE_*) -------------------------------------------------------
 * The Local Entropy ensemble: M replicas of one graph, each coupled to an explicit reference ("centre") configuration by the inner graph
 * GraphLE{M,gammaT} with gammaT = gamma / beta (LE.jl:221-225): integer fields lfields = sigma_c sigma_(i,k) on a replica site and
 * sigma_c mu_i (mu_i = sum_k sigma_(i,k)) on the centre, DeltaE0 = 2 gammaT lfields, energy(X0) = -gammaT sum_i sigma_c mu_i.  Replica k is slice k
 * of a DoubleGraph whose residual is the slice graph's delta_energy (not divided by M); centre moves have residual 0 (LE.jl:276-290).  The
 * centre graph's own energy is not part of E.  The centre and all M slices share one coupling set.
 *   N = Nk * (M + 1) spins per replica of the batch, in the reference's site order: site j (0-based) is spin i = j / (M+1) of the centre when
 *   k = j % (M+1) is 0 and of replica k otherwise (LE.jl:55-84) — in every configuration that crosses this ABI and in rrrmc_rrr_cache.
 *   3 <= M <= 31, N <= 65 535.  Energies are Float64 (_f64 entry points).
 * rrrmc_ctx_create_le: slice_kind rrrmc_re_slice; then the couplings (rrrmc_set_couplings_bits [Nk rows] for _SK, rrrmc_set_couplings_dense
 * [Nk x Nk] for _SKN, nothing for _EMPTY) and rrrmc_le_set_params.  Samplers: rrrmc_rrr_mc_async (rrrMC(X::DoubleGraph): the DeltaECache over
 * L = M/2 + 2 (M even) or (M+1)/2 (M odd) levels, classes by findk evaluated literally; fourK is ignored; streams as the Robust Ensemble's)
 * and rrrmc_standard_mc_async / rrrmc_standard_mc_f64, with the resume, debug-check, timing, results and cache entry points of the other
 * models.  rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and rrrmc_extremal_opt_async return RRRMC_ERR_UNSUPPORTED. */
RRRMC_API int32_t rrrmc_ctx_create_le(rrrmc_ctx **out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0);
/* The parameters gamma and beta_graph of GraphLocalEntropy(Nk, M, gamma, beta_graph, ...) (gammaT = gamma / beta_graph, not the sampler's beta).
 * gammaT must be finite and 2 M gammaT too; gamma = 0 is allowed.  Required before the first sampler or energy call; a change ends a resumed run. */
RRRMC_API int32_t rrrmc_le_set_params(rrrmc_ctx *ctx, double gamma, double beta_graph);
/* LEenergies(X) (LE.jl:259-269): out[R * M], energy(X1[k], C1[k]) of every replica slice of every replica of the batch for the current
 * configuration.  rrrmc_le_cenergy: cenergy(X) (LE.jl:271-274), out[R], energy(Xc, Cc) of the centre configuration under the slice graph
 * (0 for GraphEmpty).  rrrmc_le_distances: distances(X) (LE.jl:309-318), out[R * M * M], the Hamming distances between the replica
 * configurations (centre excluded), entry (k1, k2) of replica r at (r * M + k1) * M + k2.  All three read the configuration only — unlike
 * the reference's LEenergies / cenergy, they do not rebuild the slice caches, so a hook that calls them leaves the run as it was. */
RRRMC_API int32_t rrrmc_le_energies(rrrmc_ctx *ctx, double *out);
RRRMC_API int32_t rrrmc_le_cenergy(rrrmc_ctx *ctx, double *out);
RRRMC_API int32_t rrrmc_le_distances(rrrmc_ctx *ctx, int64_t *out);
/* Host-only (no device needed): dElist[L] = allDeltaE(GraphLE{M, gamma/beta}) (LE.jl:176-179), L = M/2 + 2 for even M and (M+1)/2 for odd M
 * (a buffer of M/2 + 2 entries always suffices). */
RRRMC_API int32_t rrrmc_le_tables(int64_t M, double gamma, double beta, double *dElist);

/* ---- GraphTopologicalLocalEntropy (src/graphs/TLE.jl; RRRMC_MODEL_TLE_*) -----------------------------------------
 * The Local Entropy ensemble with a second, topological coupling over the slice graph's own neighbourhoods: the inner graph
 * GraphTLE{M,gammaT,lambdaT} (gammaT = gamma / beta, lambdaT = lambda / beta, TLE.jl:390-396) keeps GraphLE's integer field lfields1 and
 *   lfields2 = sigma_(i,k) sigma_c,i sum_{i2 in d(i)} sigma_c,i2 sigma_(i2,k) on replica site (i,k), the sum of those over k on centre i,
 * with DeltaE0 = 2 gammaT lfields1 + 2 lambdaT lfields2 and energy(X0) = n gammaT + r lambdaT (integers n, r; TLE.jl:79-142, 301-311).  Sites,
 * site order, residuals, the shared coupling set and what E leaves out (the centre's own energy) are GraphLocalEntropy's.  d(i), the
 * neighbour lists, are neighbors(g0, i) of the slice graph: empty for GraphEmpty, all other sites ascending for GraphSK / GraphSKNormal,
 * neighb[i] (first-appearance order) for GraphSAT.  allDeltaE has tens to hundreds of levels: L = |unique |DeltaE1 + DeltaE2|| with
 * DeltaE2 = 2 d lambdaT for |d| <= M max|d(i)| (TLE.jl:335-347).
 *   Limits (RRRMC_ERR_UNSUPPORTED): 3 <= M <= 31 (M <= 2: RRRMC_ERR_INVALID_ARG, the reference's check), N = Nk (M+1) <= 65 535,
 *   2L <= 65 535, each slice kind's own limits, and R * 2L * N * 2 bytes of dense set storage <= 16 GiB per device.
 * rrrmc_ctx_create_tle: slice_kind RRRMC_RE_SLICE_EMPTY / _SK / _SKN / _SAT (the other kinds: RRRMC_ERR_UNSUPPORTED; 7 and values outside
 * rrrmc_re_slice: RRRMC_ERR_INVALID_ARG); then the couplings or clauses (rrrmc_set_couplings_bits, rrrmc_set_couplings_dense,
 * rrrmc_set_clauses), rrrmc_tle_set_topology and rrrmc_tle_set_params, in that order.  Samplers: rrrmc_rrr_mc_async (fourK ignored) and
 * rrrmc_standard_mc_async / rrrmc_standard_mc_f64, with the resume, debug-check, timing, results, spin and snapshot entry points of the other
 * models; rrrmc_le_energies (= TLEenergies, TLE.jl:437-453), rrrmc_le_cenergy and rrrmc_le_distances serve these contexts too.
 * rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and rrrmc_extremal_opt_async return RRRMC_ERR_UNSUPPORTED; rrrmc_rrr_cache (int8 class ids) is not
 * served: use rrrmc_tle_cache. */
RRRMC_API int32_t rrrmc_ctx_create_tle(rrrmc_ctx **out, int64_t Nk, int64_t M, int32_t slice_kind, int64_t R, int32_t device, uint32_t replica0);
/* d(i) as ordered 0-based lists in CSR form: rowptr[Nk + 1] (rowptr[0] = 0), cols[rowptr[Nk]].  The checks of TLE.jl:34-46 — entries in
 * range, no self-loop, no duplicate, symmetry — fail with RRRMC_ERR_INVALID_ARG and the reference's wording (1-based numbers) in
 * rrrmc_last_error.  A new topology ends a resumed run and asks for rrrmc_tle_set_params again.  rrrmc_tle_check_topology: the same checks
 * on the host only (no device); maxdeg_out (may be NULL) receives max |d(i)|. */
RRRMC_API int32_t rrrmc_tle_set_topology(rrrmc_ctx *ctx, const int32_t *rowptr, const int32_t *cols);
RRRMC_API int32_t rrrmc_tle_check_topology(int64_t Nk, const int32_t *rowptr, const int32_t *cols, int64_t *maxdeg_out);
/* The parameters of GraphTopologicalLocalEntropy(Nk, M, gamma, lambda, beta_graph, ...), after the topology: builds allDeltaE, and the
 * class of every (lfields1, lfields2) pair by findk evaluated literally (DeltaE.jl:26-60, :83).  gamma / beta_graph, lambda / beta_graph and
 * the largest level must be finite; zeros and negative values are allowed.  A change ends a resumed run. */
RRRMC_API int32_t rrrmc_tle_set_params(rrrmc_ctx *ctx, double gamma, double lambda, double beta_graph);
/* Host-only (no device needed): allDeltaE(GraphTLE{M, gamma/beta, lambda/beta}) for lists with max |d(i)| = maxdeg.  L_out receives its
 * length L; dElist_out (NULL: only L is written) receives the L levels. */
RRRMC_API int32_t rrrmc_tle_tables(int64_t M, double gamma, double lambda, double beta, int64_t maxdeg, double *dElist_out, int64_t *L_out);
/* The DeltaECache after the last rrrMC call: pos_out[R * N] the class a + L up of every ABI site, sizes_out[R * 2L] the set sizes (either
 * may be NULL). */
RRRMC_API int32_t rrrmc_tle_cache(rrrmc_ctx *ctx, int32_t *pos_out, int32_t *sizes_out);
/* The kernel build of the last rrrMC call: 0 none yet, 1 the chain's hot state in LDS (chosen when it fits and all R wavefronts are
 * resident at once), 2 in global memory.  RRRMC_TLE_NO_LDS=1 forces 2, RRRMC_TLE_LDS=1 forces 1 whenever the state fits. */
RRRMC_API int32_t rrrmc_tle_build(rrrmc_ctx *ctx, int32_t *build_out);
/* The same for a Robust Ensemble or Local Entropy context (rrrmc_ctx_create_re, rrrmc_ctx_create_le and their _f64 forms): the kernel
 * build of the last rrrMC call: 0 none yet, 1 one wavefront per replica with the chain's hot state (and the slices' Stabilities) in LDS,
 * chosen when they fit 160 KiB, 2 one thread per replica in global memory.  RRRMC_RE_NO_LDS=1 / RRRMC_LE_NO_LDS=1 force 2.  standardMC
 * has one build and leaves the value alone.  A multi-device context reports its first shard.  Other contexts: RRRMC_ERR_STATE. */
RRRMC_API int32_t rrrmc_ens_build(rrrmc_ctx *ctx, int32_t *build_out);

/* ---- GraphAddFields / GraphAddSubFields (src/graphs/AddFields.jl; RRRMC_MODEL_AF_*, RRRMC_MODEL_ASF_*) ------------
 * A DoubleGraph whose inner graph X0 = GraphAF(h) is a set of N independent external fields (energy(X0) = sum_i h_i sigma_i, left to
 * right; delta_energy(X0, i) = -2 sigma_i h_i; neighbors(X0, i) = ()) over any graph g of N spins:
 *   GraphAddFields    (sub = 0): E = energy(X0) + energy(g), DeltaE = DeltaE(X0) + DeltaE(g), residual = DeltaE(g);
 *   GraphAddSubFields (sub = 1): E = energy(g),              DeltaE = DeltaE(g),              residual = DeltaE(g) - DeltaE(X0):
 *     the fields only shape the proposals of rrrMC, the stationary law is g's own.
 * rrrMC(X::DoubleGraph) runs over DeltaECacheCont + DynamicSampler on X0 (src/DeltaE.jl:297-410, src/DynamicSamplers.jl): X0 has no
 * neighbours, so a move is one setindex!, O(log N) whatever g is.  Integer energies of g enter as exact Float64s; results through
 * rrrmc_fetch_results_f64.
 *   g, by its rrrmc_re_slice kind and with that kind's own upload call and limits: GraphEmpty (nothing to upload), binary GraphSK
 *   (rrrmc_set_couplings_bits), GraphSKNormal (rrrmc_set_couplings_dense), GraphPercStep / GraphPercLinear (rrrmc_set_patterns; N odd,
 *   N <= 32 767), GraphCommStep / GraphCommReLU / GraphCommQu (rrrmc_set_comm_patterns with the creator's K2; N = K1*K2 with each kind's
 *   parities, N <= 32 767), GraphSAT (rrrmc_set_clauses; N <= 65 535), GraphPercXEntr (rrrmc_set_patterns and rrrmc_set_loss_table; N odd,
 *   N <= 32 767).  N <= 65 535 for the first three.  N = 1 runs (a tree of no levels).
 *   K2 is read for the committee machines only.
 * rrrmc_ctx_create_af, then g's upload, then rrrmc_af_set_fields.  Samplers: rrrmc_rrr_mc_async (fourK ignored; staged_thr = 0.5 is the
 * reference's default for a DoubleGraph) and rrrmc_standard_mc_async / rrrmc_standard_mc_f64 (the common SITE / ACCEPT_F64 streams), with
 * the resume, debug-check, timing, results, rrrmc_rrr_stats, rrrmc_energy_f64, rrrmc_tracked_energy_f64, spin, snapshot and overlap entry
 * points of the other models.  rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and rrrmc_extremal_opt_async return RRRMC_ERR_UNSUPPORTED.
 * A draw of the sampler that lands on an element of weight 0 (or beyond N) refreshes the tree once; if that happens with nothing to
 * refresh, the reference's "Unrecoverable loss of precision detected in the dynamic sampler" is reported by the next rrrmc_sync / fetch
 * (RRRMC_ERR_STATE). */
RRRMC_API int32_t rrrmc_ctx_create_af(rrrmc_ctx **out, int32_t slice_kind, int32_t sub, int64_t N, int64_t K2, int64_t R, int32_t device,
                                      uint32_t replica0);
/* The fields h[N] (the same for every replica).  Non-finite entries: RRRMC_ERR_INVALID_ARG.  New fields end a resumed run. */
RRRMC_API int32_t rrrmc_af_set_fields(rrrmc_ctx *ctx, const double *h);
/* The kernel build of the last rrrMC call: 0 none yet, 1 the sampler's tree, DeltaEs, the spins and g's per-chain state in LDS (chosen
 * whenever they fit 160 KiB), 2 in global memory.  RRRMC_AF_NO_LDS=1 forces 2.  Both builds give the same bits. */
RRRMC_API int32_t rrrmc_af_build(rrrmc_ctx *ctx, int32_t *build_out);
/* The DeltaECacheCont after the last rrrMC call: dEs_out[R * N] = DeltaEs, v_out[R * N] the sampler's weights, z_out[R], trefresh_out[R]
 * (any may be NULL). */
RRRMC_API int32_t rrrmc_af_cache(rrrmc_ctx *ctx, double *dEs_out, double *v_out, double *z_out, int64_t *trefresh_out);

/* ---- GraphMixed (src/graphs/Mixed.jl; RRRMC_MODEL_MIXED, RRRMC_MODEL_MIXED_AF, RRRMC_MODEL_MIXED_ASF) ------
 * rrrmc_ctx_create_mixed: R chains of GraphMixed(graphs...) on N spins, or of a field wrapper over it.  kinds[nkinds] lists the 2 .. 7
 * components in order, each RRRMC_RE_SLICE_EMPTY, _SK, _SKN, _PERC_STEP, _PERC_LINEAR, _PERC_XENTR, _COMM_STEP, _COMM_RELU, _COMM_QU, _SAT
 * or _SPARSE_F64.  wrap: 0 GraphMixed itself, 1 GraphAddFields(h, mixed), 2 GraphAddSubFields(h, mixed).  K is read for a _SPARSE_F64
 * component (1 <= K <= 8), K2 for a committee machine.  A context holds one upload of each storage group -- {SK}, {SKN}, {PERC_STEP,
 * PERC_LINEAR, PERC_XENTR}, {COMM_STEP, COMM_RELU, COMM_QU}, {SAT}, {SPARSE_F64} -- so a second component of one group is
 * RRRMC_ERR_UNSUPPORTED (the message names the group); _EMPTY may repeat.  N <= 65535, and every component's own limits (perceptrons and
 * committee machines N <= 32767 and their parities, whose message names the component).  Then each component's upload call, in any order
 * (rrrmc_set_couplings_bits, _dense, rrrmc_set_patterns and rrrmc_set_loss_table, rrrmc_set_comm_patterns, rrrmc_set_clauses,
 * rrrmc_set_graph_f64), and rrrmc_af_set_fields for wrap 1 or 2; a sampling or energy call before that answers RRRMC_ERR_STATE and names the
 * missing call.  energy = the left-to-right Float64 sum of the components' energies, delta_energy the left-to-right sum of theirs
 * (Mixed.jl:33-40): the order of the list is part of the model.  Results through the Float64 entry points (integers as exact doubles).
 * Samplers: rrrmc_standard_mc_async on all three models; rrrmc_rrr_mc_async on wrap 1 and 2 (RRRMC_ERR_UNSUPPORTED on wrap 0, as on the
 * other stand-alone dense graphs); bklMC / wtmMC / extremal_opt RRRMC_ERR_UNSUPPORTED.  rrrmc_set_resume, rrrmc_set_debug_checks, timing,
 * rrrmc_energy_f64 / rrrmc_tracked_energy_f64, spins, snapshots and overlaps as for rrrmc_ctx_create_af; rrrmc_af_cache / rrrmc_af_build
 * on wrap 1 and 2.  rrrmc_ctx_create_mixed_multi makes the same context over several devices (shards as rrrmc_ctx_create_multi's). */
RRRMC_API int32_t rrrmc_ctx_create_mixed(rrrmc_ctx **out, const int32_t *kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2,
                                         int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_ctx_create_mixed_multi(rrrmc_ctx **out, const int32_t *kinds, int32_t nkinds, int32_t wrap, int64_t N, int64_t K, int64_t K2,
                                               int64_t R, const int32_t *device_ids, int32_t ndev, uint32_t replica0);
/* E_out[R * nkinds]: energy(graphs[c], C) of every component of the live configuration of every chain, recomputed from the configuration
 * (read-only: a run the context continues is not disturbed).  Their left-to-right sum is energy(GraphMixed, C). */
RRRMC_API int32_t rrrmc_mixed_energies(rrrmc_ctx *ctx, double *E_out);
/* Which build the last rrrmc_standard_mc_async call on a mixed context ran (the first shard of a multi-device context): 0 none yet, 1 one
 * thread per chain, 2 one wavefront per chain.  Up to 16384 chains run the wave build; RRRMC_MIXED_NO_WAVE=1 / RRRMC_MIXED_WAVE=1 force a
 * build; the builds give the same bits. */
RRRMC_API int32_t rrrmc_mixed_build(rrrmc_ctx *ctx, int32_t *build_out);

/* ---- The regular 3-spin model (src/graphs/PSpin3.jl; RRRMC_MODEL_PSPIN3, RRRMC_MODEL_PSPIN3_AF, RRRMC_MODEL_PSPIN3_ASF) ------
 * rrrmc_ctx_create_pspin3: R chains of GraphPSpin3(N, K) -- K layers, each a partition of the N sites into N / 3 triples, all couplings
 * +1 -- or of a field wrapper over it.  wrap: 0 the graph itself, 1 GraphAddFields(h, g), 2 GraphAddSubFields(h, g).  Limits: N <= 65535
 * (16-bit site ids), N % 3 == 0, 1 <= K <= 16; RRRMC_ERR_UNSUPPORTED beyond.  Spins: one BitVector of N bits per chain (chunks of 64).
 * rrrmc_set_pspin3: the partner table A[N][2K], 0-based: A[i][2k], A[i][2k+1] are the two partners of i in layer k (PSpin3.jl:32-43).
 * Checked: every id in range; the two partners of a slot distinct and different from i; for slot k of i = (y, z), y's list holds the pair
 * {i, z} and z's list the pair {i, y} as often as i's holds {y, z} (a pair that two layers share counts twice).  A malformed table is
 * RRRMC_ERR_INVALID_ARG.  Then rrrmc_af_set_fields for wrap 1 or 2.
 * energy = -(sum over the triples of the product of the three spins), delta_energy(i) = 2 (2c - K) with c the layers whose triple has the
 * product +1: integers, reported through the Float64 entry points as exact doubles; recomputed from the spins (the reference's
 * LocalFields{Int} is an exact function of the configuration).
 * Samplers.  wrap 0: rrrmc_standard_mc_async (the SITE / ACCEPT_F64 streams and det_exp; every beta but NaN -- beta = +inf with
 * delta_energy = 0 is rejected, as in the reference); rrrmc_rrr_mc_async, rrrmc_bkl_mc_async, rrrmc_wtm_mc_async and rrrmc_extremal_opt_async
 * answer RRRMC_ERR_UNSUPPORTED and name the field wrappers as the way to run rrrMC.  wrap 1 and 2: rrrmc_rrr_mc_async and
 * rrrmc_standard_mc_async as on every context of rrrmc_ctx_create_af (rrrmc_af_cache, rrrmc_af_build too).  rrrmc_set_resume,
 * rrrmc_set_debug_checks (the tracked E against the energy of the configuration), timing, rrrmc_energy_f64 / rrrmc_tracked_energy_f64,
 * spins, seeds and rrrmc_ctx_create_multi as for rrrmc_ctx_create_sat.
 * rrrmc_pspin_build: the kernel build of the last standardMC call on wrap 0 (the first shard of a multi-device context): 0 none yet, 1 one
 * thread per chain, 2 one wavefront per chain (64 consecutive iterations side by side, retired in the chain's order).  Up to 16384 chains
 * run the wave build (the two cross between 16384 and 32768 chains, profiles/r20/pspin3.md); RRRMC_PSPIN_NO_WAVE=1 / RRRMC_PSPIN_WAVE=1
 * force a build; the builds give the same bits. */
RRRMC_API int32_t rrrmc_ctx_create_pspin3(rrrmc_ctx **out, int64_t N, int64_t K, int32_t wrap, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_set_pspin3(rrrmc_ctx *ctx, const int32_t *A);
RRRMC_API int32_t rrrmc_pspin_build(rrrmc_ctx *ctx, int32_t *build_out);
/* The constructor's K randperm(N) (PSpin3.jl:32-43; the reference's rand is unpinned) on a Philox stream of its own (PSPIN = 13): layer k
 * is the Fisher-Yates shuffle l = 0 .. N-1; for j = N-1 down to 1: swap(l[j], l[floor(u64 * (j+1) / 2^64)]) with the draws k (N-1) + (N-1-j)
 * of the stream; consecutive threes of l are the triples (v1, v2, v3): v1 lists (v2, v3), v2 (v1, v3), v3 (v1, v2).  A_out[N][2K], 0-based.
 * A host function: no device is touched. */
RRRMC_API int32_t rrrmc_gen_pspin3(int64_t N, int64_t K, uint64_t seed, int32_t *A_out);

/* rrrMC(X::DoubleGraph, beta, iters; step, staged_thr, staged_thr_fact) (src/RRRMC.jl:221-290) for all R replicas.
 *   fourK = round(2/beta * log(coth(beta * Gamma / M)), digits = 8)  (QT.jl:165) is computed by the caller.
 * Enqueues on the ctx's stream; rrrmc_sync + rrrmc_fetch_results_f64 return Es [R x iters/step] and accepted [R];
 * rrrmc_rrr_stats adds the number of staged iterations per replica ("frac. staged iters", RRRMC.jl:287). */
RRRMC_API int32_t rrrmc_rrr_mc_async(rrrmc_ctx *ctx, double beta, double fourK, int64_t iters, int64_t step,
                                     double staged_thr, double staged_thr_fact);
RRRMC_API int32_t rrrmc_rrr_stats(rrrmc_ctx *ctx, int64_t *staged_iters_out);
/* rrrmc_rrr_mc_async also serves rrrMC(X::SingleGraph, ...) (src/RRRMC.jl:149-219): on RRRMC_MODEL_SPARSE_PM1 with the
 * integer-level DeltaECache{Int,L} (fourK ignored, results through rrrmc_fetch_results), on RRRMC_MODEL_SK_NORMAL with
 * DeltaECacheCont + DynamicSampler (src/DeltaE.jl:297-410, src/DynamicSamplers.jl; results through rrrmc_fetch_results_f64).
 * On RRRMC_MODEL_SPARSE_F64 (GraphRRGNormal / GraphEANormal) rrrmc_rrr_mc_async, rrrmc_bkl_mc_async and rrrmc_wtm_mc_async run the
 * continuous-energy versions (DeltaECacheCont + DynamicSampler, THeap; results through rrrmc_fetch_results_f64); rrrmc_bkl_mc_async
 * also serves RRRMC_MODEL_SK_NORMAL.  RRRMC_MODEL_SK_BINARY (GraphSK, a SimpleGraph{Float64} too: SK.jl:28) runs rrrMC / bklMC / wtmMC
 * through the same continuous-energy caches over delta_energy = lfields[i] / sqrt(N) (SK.jl:137-140).
 * bklMC(X, beta, iters; step) (src/RRRMC.jl:311-359) on RRRMC_MODEL_SPARSE_PM1: rejection-free Bortz-Kalos-Lebowitz sampler;
 * `iters` counts the skipped rejections too; rrrmc_rrr_stats then returns the number of moves actually made ("true it"). */
RRRMC_API int32_t rrrmc_bkl_mc_async(rrrmc_ctx *ctx, double beta, int64_t iters, int64_t step);
/* wtmMC(X, beta, samples; step) (src/RRRMC.jl:376-426, src/WaitingTimes.jl) on RRRMC_MODEL_SPARSE_PM1: the waiting-time
 * method.  `step` is in sweeps (it is divided by N like RRRMC.jl:391); `samples` energies are taken at global times k*step/N.
 * rrrmc_sync + rrrmc_fetch_results return Es [R x samples] and, as `accepted`, num_moves; rrrmc_wtm_times the final global time
 * of every replica ("global time", RRRMC.jl:421). */
RRRMC_API int32_t rrrmc_wtm_mc_async(rrrmc_ctx *ctx, double beta, int64_t samples, double step);
RRRMC_API int32_t rrrmc_wtm_times(rrrmc_ctx *ctx, double *t_out);
/* extremal_opt(X, tau, iters; step) (src/RRRMC.jl:474-521) on RRRMC_MODEL_SPARSE_PM1, EOCache{Int,L} (src/DeltaE.jl:412-555).
 *   ftau[N] = cumsum(j^-tau, j = 1..N), computed by the caller as the reference does at DeltaE.jl:444-445.
 * rrrmc_sync + rrrmc_fetch_results return the energies the hook would see (E at iterations k*step, before the move; `accepted`
 * is not meaningful); rrrmc_extremal_opt_results returns Emin[R], Cmin (R x ceil(N/64) chunks) and itmin[R]; the final
 * configuration is read with rrrmc_get_spins. */
RRRMC_API int32_t rrrmc_extremal_opt_async(rrrmc_ctx *ctx, const double *ftau, int64_t iters, int64_t step);
RRRMC_API int32_t rrrmc_extremal_opt_results(rrrmc_ctx *ctx, int64_t *Emin_out, uint64_t *Cmin_chunks, int64_t *itmin_out);
/* The same call on the graphs that are not DiscrGraphs — RRRMC_MODEL_SPARSE_F64 (GraphRRGNormal / GraphEANormal) and
 * RRRMC_MODEL_SPARSE_DISCRETIZED (the DoubleGraphs) — runs the reference's generic cache, EOCacheCont (src/DeltaE.jl:557-635): the
 * ranking of all spins by delta_energy is re-established after every flip (the kernel slides the K + 1 changed entries to their
 * places instead of re-sorting) and every run of EQUAL values is put in a fresh uniformly random order per move (rankshuffle!,
 * :611-634; the library's restatement: order by a per-(move, site) Philox key).  N <= 65 535.  RRRMC_MODEL_SK_NORMAL and
 * RRRMC_MODEL_SK_BINARY run it too (every spin a neighbour: the ranking is re-sorted at every flip; N <= 4096).  Energies are Float64:
 * rrrmc_fetch_results_f64, and rrrmc_extremal_opt_results_f64 for (Emin, Cmin, itmin). */
RRRMC_API int32_t rrrmc_extremal_opt_results_f64(rrrmc_ctx *ctx, double *Emin_out, uint64_t *Cmin_chunks, int64_t *itmin_out);
/* parity/debug view of the move-selection cache after the last rrrMC call: pos_out[R * N] = class of every spin
 * (DeltaECache.pos, 0-based a + 2*up), sizes_out[R * 4] = |class k| (DeltaE.jl:63-73).  RRRMC_MODEL_RE_*: class a + L*up of every site j,
 * sizes_out[R * 2L] with L = ceil(M/2); RRRMC_MODEL_LE_*: the same with L = M/2 + 2 (M even) or (M+1)/2 (M odd).  RRRMC_MODEL_SPARSE_PM1 / _LEVELS (rrrMC and
 * bklMC; class a + L*up) and RRRMC_MODEL_SPARSE_DISCRETIZED: sizes_out[R * 16], class k of replica r at 16 r + k. */
RRRMC_API int32_t rrrmc_rrr_cache(rrrmc_ctx *ctx, int8_t *pos_out, int32_t *sizes_out);

/* Opt-in FAST standardMC for RRRMC_MODEL_SPARSE_F64 (GraphRRGNormal / GraphEANormal, K <= 4, N <= 8192): replicas bit-sliced and
 * resident in LDS as for the +-J models, no stored fields — delta_energy takes 2^K values per site, so the accept test runs against
 * per-site threshold tables.  Same SITE stream as rrrmc_standard_mc_async; the acceptance uniforms come from the ACCEPT bit-plane stream
 * (as the +-J models) instead of ACCEPT_F64, and delta_energy is the pattern sum 2 sum_k +-|J_ik| instead of the incrementally
 * updated cache (last-bit differences), so the chain is NOT the one rrrmc_standard_mc_async produces; it is a faithful standardMC
 * chain with its own oracle restatement (configurations / accepted counts identical to it, energies — re-evaluated at every sample —
 * within 1e-9 relative).  Two orders of magnitude faster.  Results: rrrmc_sync + rrrmc_fetch_results_f64. */
RRRMC_API int32_t rrrmc_standard_mc_fast_async(rrrmc_ctx *ctx, double beta, int64_t iters, int64_t step);

/* Resumed standardMC calls.  A reference call keeps its incrementally updated cache and its tracked energy E from the first to the last
 * iteration, hook calls included (src/RRRMC.jl:95-118); a library call starts, like a fresh reference call, from E = energy(X, C) and a
 * rebuilt cache (:95).  For the integer models the two coincide; for the Float64 models (RRRMC_MODEL_SK_NORMAL / SK_BINARY / SPARSE_F64 /
 * SPARSE_DISCRETIZED, standardMC on a GraphQuant) the last bits differ.  rrrmc_set_resume(ctx, 1): every following standardMC call that
 * finds the state left by a previous standardMC call (no rrrmc_set_spins / rrrmc_init_spins_random / other sampler in between) continues
 * from it — tracked energy, local fields, undo record, move_last — so that a run cut into pieces at the hook points is bit for bit the
 * run made in one call.  rrrmc_tracked_energy_f64 reads that tracked energy (what the reference hands to its hook), R doubles. */
RRRMC_API int32_t rrrmc_set_resume(rrrmc_ctx *ctx, int32_t on);
/* Resumed rrrMC / bklMC / wtmMC / extremal_opt calls — the hook of every sampler (src/RRRMC.jl:152,186 · :224,255 · :314,341 · :379,404 · :477,501).
 * A reference call keeps its whole chain in local variables from the first to the last iteration, hook calls included: the move-selection
 * cache (DeltaECache: the ArraySets in member order, T, z — src/DeltaE.jl:63-73; DeltaECacheCont: the DynamicSampler's tree and its refresh
 * countdown — src/DynamicSamplers.jl:18-33; THeap and the global time — src/WaitingTimes.jl; EOCache / EOCacheCont: the ranking), the graph's
 * own cache, the tracked E, the acc_rate average of rrrMC, `it` / `nextstep` of bklMC, Emin / Cmin / itmin of extremal_opt.  With
 * rrrmc_set_resume(ctx, 1), a call of one of these samplers that finds the RUN left by a previous call of the SAME sampler with the SAME
 * parameters (beta, fourK, staged_thr, staged_thr_fact; bklMC: step; wtmMC: step; extremal_opt: ftau) — and nothing in between that changes
 * the configuration, the disorder, the seed or the caches (rrrmc_set_spins, rrrmc_init_spins_random, rrrmc_seed, rrrmc_set_graph*,
 * rrrmc_energy*, rrrmc_get_fields, any other sampler) — CONTINUES that run instead of starting one (energy(X, C) + a fresh cache):
 *   - the run's iteration counter carries on: samples are taken before the iterations that are multiples of `step` of the RUN's count
 *     (a first call of step - 1 iterations takes none; the next call of `step` iterations takes one before its first move), extremal_opt's
 *     itmin counts from the start of the run;
 *   - bklMC: `iters` more iterations are allowed; `it`, `nextstep` and the pending (skip, move) draw carry on — a call of `step` iterations
 *     ends at the next sample point, with the configuration, E and accepted count the reference hands to its hook there (:336-341);
 *     the reference's loop ends with its LAST SAMPLE (:340-343: the iterations between it and `iters` are never made), so a resumed call
 *     whose allowance does not reach the run's next sample point makes no move;
 *   - wtmMC: `samples` more samples; the heap, the global time and `nextstep` carry on (:399-404);
 *   - rrrmc_fetch_results* / rrrmc_rrr_stats return the samples and the accepted / staged counts of the CALL.
 * A run cut into calls anywhere is bit for bit the run made in one call — energies, configurations, counts and the cache — through every
 * kernel build (the LDS-resident ones write their state back at the end of a call and read it at the start of the next).
 * rrrmc_tracked_energy / _f64 read the tracked E without disturbing the run; rrrmc_get_spins, rrrmc_rrr_cache, rrrmc_wtm_times,
 * rrrmc_extremal_opt_results*, the snapshot and observable calls do not disturb it either.
 * rrrmc_tracked_energy: the integer models' tracked energy (level units), R values. */
RRRMC_API int32_t rrrmc_tracked_energy(rrrmc_ctx *ctx, int64_t *E_out);
/* Debug mode: the reference's latent consistency checks as a switch a user can turn on (its commented-out asserts in update_cache!,
 * src/graphs/RRG.jl:229-231, SK.jl:125-130, 268-273, and its test suite's hook, test/runtests.jl:12-20).  on != 0: after EVERY standardMC
 * call the library recomputes energy(X, C) of every replica from the configuration on the device and compares it with the energy the
 * sampler tracked (exactly for RRRMC_MODEL_SPARSE_PM1; within 1e-10 N for RRRMC_MODEL_SK_NORMAL, where the cached local fields are
 * compared with recomputed ones too); the following rrrmc_sync (or any synchronous call) returns RRRMC_ERR_STATE and names a replica
 * if any value differs.  Costs one energy evaluation per call; off by default. */
RRRMC_API int32_t rrrmc_set_debug_checks(rrrmc_ctx *ctx, int32_t on);
RRRMC_API int32_t rrrmc_tracked_energy_f64(rrrmc_ctx *ctx, double *E_out);

/* Timing of the last sampling call measured with HIP events on the ctx's stream:
 *   total_ms   first planner launch -> last sweep kernel end
 *   sweep_ms   sum of the sweep (dominant) kernel's durations,  sweep_launches = how many launches */
RRRMC_API int32_t rrrmc_last_timing(rrrmc_ctx *ctx, double *total_ms, double *sweep_ms, int32_t *sweep_launches);
/* Accumulated kernel timing over MANY queued async calls (RRRMC_MODEL_SPARSE_PM1 standardMC): rrrmc_timing_accumulate(ctx, 1)
 * gives every sweep launch of every following sampling call its own HIP-event pair (both calls synchronise the stream; the
 * sampling calls in between stay asynchronous); rrrmc_timing_total returns the summed duration of those launches and their count.
 * rrrmc_timing_accumulate(ctx, 0) returns to the per-call bookkeeping of rrrmc_last_timing.  on > 1 additionally creates the event
 * pairs of the first `on` launches right away, so that a timed region of queued calls performs no event creation. */
RRRMC_API int32_t rrrmc_timing_accumulate(rrrmc_ctx *ctx, int32_t on);
RRRMC_API int32_t rrrmc_timing_total(rrrmc_ctx *ctx, double *sweep_ms, int64_t *sweep_launches);

/* The build of spf_team_kernel<K, waves, slots, width> the default standardMC of a RRRMC_MODEL_SPARSE_F64 context launches on its device
 * (teams of `width` replicas, `waves` wavefronts and `slots` in-flight records each); zeros when the one-wavefront kernel runs instead.
 * A reporting helper (bench.py names the kernel its measured traffic belongs to); any output may be NULL. */
RRRMC_API int32_t rrrmc_spf_team_build(rrrmc_ctx *ctx, int32_t *waves_out, int32_t *width_out, int32_t *slots_out);
/* Samples per replica the last sampling call took: the row length of rrrmc_fetch_results*' Es_out.  iters / step for a call that starts a
 * run; a RESUMED call takes a sample before every iteration that is a multiple of `step` of the run's count (see rrrmc_set_resume). */
RRRMC_API int64_t rrrmc_results_samples(const rrrmc_ctx *ctx);
/* Iterations consumed from the current seed's streams so far. */
RRRMC_API int64_t rrrmc_iterations_done(const rrrmc_ctx *ctx);

/* ---- Float64-coupling sparse models (RRRMC_MODEL_SPARSE_F64) ---------------------------
 * GraphRRGNormal / GraphEANormal: SimpleGraph{Float64} on the neighbour table of GraphRRG / GraphEA.  Create with
 * rrrmc_ctx_create(model = RRRMC_MODEL_SPARSE_F64, N, K, R); K <= 8.  A [N x K] 0-based with ascending rows (a neighbour may
 * repeat: EA with L = 2, handled through the de-duplicated list like EA.jl:613-653), J [N x K] Float64, symmetric.
 * Energies / fields / results through the _f64 entry points; sampler: rrrmc_standard_mc_async / rrrmc_standard_mc_f64.
 * Replaces GraphRRGNormal{K}(N) (RRG.jl:503-520), GraphEANormal{twoD}(L, A, J) (EA.jl:539-552). */
RRRMC_API int32_t rrrmc_set_graph_f64(rrrmc_ctx *ctx, const int32_t *A, const double *J);
/* gen_J(Float64, N, A) do randn() end (RRG.jl:71-96, EA.jl:45-71): one GAUSS-stream normal per bond. J_out[N*K]. */
RRRMC_API int32_t rrrmc_gen_couplings_gauss(int64_t N, int64_t K, const int32_t *A, uint64_t seed, double *J_out);
/* gen_J(Float64, N, A) do lo + (hi - lo) * rand() end — the aliases over GraphEANormal draw 4 * rand() - 2 (src/QAliases.jl:60-62,
 * src/REAliases.jl:53-55): the bond visiting order of rrrmc_gen_couplings_gauss (x < y in table order, mirrored into the first free slot of
 * row y), draw n = the 53-bit uniform of Philox block n of the UNIFORM stream (the reference's rand is unpinned: the stream is ours).
 * lo, hi finite, lo < hi.  J_out[N*K].  Needs no device. */
RRRMC_API int32_t rrrmc_gen_couplings_uniform(int64_t N, int64_t K, const int32_t *A, uint64_t seed, double lo, double hi, double *J_out);

/* ---- The three ensembles over sparse Float64 slices (RRRMC_MODEL_RE_SPARSE_F64 / _LE_ / _TLE_; RRRMC_RE_SLICE_SPARSE_F64) ------
 * GraphEARE / GraphEALE / GraphEATLE (src/REAliases.jl:43-75, src/LEAliases.jl:43-75, src/TLEAliases.jl:36-68) and the generic constructors
 * over a GraphEANormal or GraphRRGNormal: every slice (and the centre of the two Local Entropy ensembles) is the one graph (A, J) of Nk sites
 * with K table entries per site.  A slice keeps its graph's LocalFields{Float64} cache (EA.jl:584-653): the residual of a move is
 * delta_energy(X1[k], C1[k], i) = -lfields[i], not divided by M; update_cache! follows every flip, and the immediate undo of a rejected
 * rrrMC move takes its move_last path, which restores the fields bit for bit.  The centre's cache is never updated.
 *   The creators are rrrmc_ctx_create_re / _le / _tle with a K: 1 <= K <= 8 as rrrmc_ctx_create_quant_f64, and the ensembles' own limits
 *   (3 <= M <= 32 for the Robust Ensemble, <= 31 for the other two, N <= 65 535).  Then rrrmc_set_graph_f64(ctx, A[Nk x K], J[Nk x K])
 *   with the checks it applies to a GraphQEAT (ascending rows, no self-loop, finite J, every bond from both ends; a neighbour may repeat:
 *   L = 2); new couplings end a resumed run.  Then rrrmc_re_set_params / rrrmc_le_set_params, or rrrmc_tle_set_topology and
 *   rrrmc_tle_set_params in that order: the topology of a GraphEATLE is neighbors(g0, i) = the distinct entries of row A[i], ascending
 *   (EA.jl:680, TLE.jl:394), which the caller computes.  Samplers and every other entry point as for the other slice kinds. */
RRRMC_API int32_t rrrmc_ctx_create_re_f64(rrrmc_ctx **out, int64_t Nk, int64_t K, int64_t M, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_ctx_create_le_f64(rrrmc_ctx **out, int64_t Nk, int64_t K, int64_t M, int64_t R, int32_t device, uint32_t replica0);
RRRMC_API int32_t rrrmc_ctx_create_tle_f64(rrrmc_ctx **out, int64_t Nk, int64_t K, int64_t M, int64_t R, int32_t device, uint32_t replica0);

/* ---- DoubleGraphs with discretised Gaussian couplings (RRRMC_MODEL_SPARSE_DISCRETIZED) --------
 * GraphRRGNormalDiscretized{Int,LEV,K} / GraphEANormalDiscretized{Int,LEV,2D}: couplings cJ ~ Normal(0,1) split by
 * discretize (src/Common.jl:38-72) into integer levels dJ (the inner DiscrGraph X0, which drives the DeltaECache) and
 * Float64 residuals rJ.  Create with rrrmc_ctx_create(model = RRRMC_MODEL_SPARSE_DISCRETIZED, N, K, R); N <= 2^28, K <= 8.
 *   lev[nlev]  the levels (distinct integers in -127..127; allΔE(X0) must have <= 8 values)
 *   ea_form    0: GraphRRG conventions (neighbors = non-zero couplings, RRG.jl:133), 1: GraphEA (repeats removed, EA.jl:158)
 * Sampler: rrrmc_rrr_mc_async (rrrMC(X::DoubleGraph), src/RRRMC.jl:221-290; fourK ignored); results through
 * rrrmc_fetch_results_f64 / rrrmc_rrr_stats; rrrmc_rrr_cache returns pos[R*N] and sizes[R*16] (class k of replica r at 16 r + k, k < 2L); energy through rrrmc_energy_f64.
 * rrrmc_bkl_mc_async / rrrmc_wtm_mc_async run bklMC / wtmMC with the continuous-energy caches over the whole graph (a DoubleGraph
 * is not a DiscrGraph: DeltaE.jl:315) and neighbors(X, i) = A[i] (RRG.jl:499) / uA[i] (EA.jl:529).
 * rrrmc_standard_mc_async / rrrmc_standard_mc_f64 run standardMC (src/RRRMC.jl:81-127) with
 * delta_energy = convert(Float64, dE0 + dE1) (RRG.jl:493-497, EA.jl:523-527).
 *
 * Level units.  The reference's level type is Int or DFloat64 (src/DFloats.jl:11-36: the Int64 t = round(x * 10^5) whose
 * Float64 value is t / 10^5; Float64 LEV tuples are mapped to it, RRG.jl:324, EA.jl:357).  lev[] and dJ[] are integer *units*;
 * wherever the reference promotes a level quantity to Float64 the library computes (units * mul) / div, with (mul, div) set by
 * rrrmc_set_level_scale: (1, 1.0) for Int levels (the default), (g, 1e5) for DFloat64 levels with units = t / g, g = gcd of
 * the levels' t.  Call it before rrrmc_energy_f64 / the samplers; rrrmc_discretize_scaled is the matching discretize. */
RRRMC_API int32_t rrrmc_set_graph_discretized(rrrmc_ctx *ctx, const int32_t *A, const int8_t *dJ, const double *rJ,
                                              const int32_t *lev, int32_t nlev, int32_t ea_form);
RRRMC_API int32_t rrrmc_set_level_scale(rrrmc_ctx *ctx, int64_t mul, double div);
/* discretize(cvec, LEV) (src/Common.jl:38-72): d_out[n] levels (units), r_out[n] residuals. */
RRRMC_API int32_t rrrmc_discretize(const double *x, int64_t n, const int32_t *lev, int32_t nlev, int8_t *d_out, double *r_out);
RRRMC_API int32_t rrrmc_discretize_scaled(const double *x, int64_t n, const int32_t *lev, int32_t nlev, int64_t mul, double div,
                                          int8_t *d_out, double *r_out);

/* ---- stand-alone GraphRRG / GraphEA with general levels (RRRMC_MODEL_SPARSE_LEVELS) ----------
 * GraphRRG{ET,LEV,K}(A, J) / GraphEA{ET,LEV,2D}(A, J) with any levels (the reference's tests use (-1,0,1), (-1.0,0.0,1.0), ...:
 * test/runtests.jl:36-60); LEV = (-1, 1) has its own bit-sliced context, RRRMC_MODEL_SPARSE_PM1.  Create with
 * rrrmc_ctx_create(model = RRRMC_MODEL_SPARSE_LEVELS, N, K, R); N <= 2^28, K <= 8, allΔE(X) <= 8 values.
 *   J[N*K], lev[nlev]   integer level units in -127..127 (rrrmc_set_level_scale gives their value: Int levels (1, 1.0), DFloat64
 *                       levels (g, 1e5), see above); ea_form as for rrrmc_set_graph_discretized
 * Samplers: rrrmc_standard_mc_async (SITE stream + ACCEPT_F64 stream: rand53 < exp(-beta dE)), rrrmc_rrr_mc_async (rrrMC(X::SingleGraph),
 * fourK ignored), rrrmc_bkl_mc_async, rrrmc_wtm_mc_async, rrrmc_extremal_opt_async.  Energies (rrrmc_energy, rrrmc_fetch_results,
 * rrrmc_extremal_opt_results) are int64 level units — exactly the reference's Int / DFloat64 payload divided by g. */
RRRMC_API int32_t rrrmc_set_graph_levels(rrrmc_ctx *ctx, const int32_t *A, const int8_t *J, const int32_t *lev, int32_t nlev, int32_t ea_form);
/* gen_J with rand(vLEV) (RRG.jl:71-96, EA.jl:45-71): COUPLING stream, J_out[N*K] in the units of lev[]. */
RRRMC_API int32_t rrrmc_gen_couplings_lev(int64_t N, int64_t K, const int32_t *A, uint64_t seed, const int32_t *lev, int32_t nlev, int8_t *J_out);

/* ---- snapshots and observables -------------------------------------------------------
 * The reference's scripts keep a copy of C.s at every hook call (scripts/scripts.jl:56-66, to_mat :13-21) and later
 * compute time overlaps with pm1dot (:283-295, parseovs :368-405).  Here the copies stay in HBM (a "snapshot" = the
 * context's spin buffer in its native layout) and the popcounts run on the device.
 *   rrrmc_snapshot_reserve  (re)allocates room for nslots snapshots (drops existing ones)
 *   rrrmc_snapshot_store    copies the live configuration into `slot` (device-to-device, on the ctx's stream)
 *   rrrmc_snapshot_get      returns slot as R x ceil(N/64) BitVector chunks, like rrrmc_get_spins (the BitMatrix column dump)
 *   rrrmc_overlaps          q_out[p * R + r] = pm1dot(replica r in slotA[p], replica r in slotB[p]) = N - 2|a xor b|;
 *                           slot -1 names the live configuration */
RRRMC_API int32_t rrrmc_snapshot_reserve(rrrmc_ctx *ctx, int32_t nslots);
RRRMC_API int32_t rrrmc_snapshot_store(rrrmc_ctx *ctx, int32_t slot);
RRRMC_API int32_t rrrmc_snapshot_get(rrrmc_ctx *ctx, int32_t slot, uint64_t *chunks);
RRRMC_API int32_t rrrmc_overlaps(rrrmc_ctx *ctx, int64_t npairs, const int32_t *slotA, const int32_t *slotB, int32_t *q_out);
/* Overlaps between DIFFERENT replicas of the stored configurations: the order-parameter distribution P(q) of the R chains on one sample,
 * and parsexovs / stats_overlaps (scripts/scripts.jl:407-457, :459-522) with two replicas as the two runs.  Every distinct slot a call
 * names is brought once to R x ceil(N/64) BitVector chunks on the device; one tiled xor-popcount kernel serves all layouts.
 *   rrrmc_cross_overlaps  q_out[(p * nA + i) * nB + j] = pm1dot(replica a0 + i of slotA[p], replica b0 + j of slotB[p]);
 *                         slot -1 names the live configuration; 0 <= a0, nA >= 1, a0 + nA <= R, likewise b0, nB
 *   rrrmc_overlap_hist    hist_out[d], d = 0..N: the number of counted replica pairs at Hamming distance d (q = N - 2d), summed over the
 *                         npairs slot pairs; hist_out is overwritten, not accumulated.  A pair with slotA[p] == slotB[p] counts
 *                         r1 < r2 (R(R-1)/2 pairs), one with different slots every r1 != r2 (R(R-1) pairs); r1 == r2, the two-time
 *                         self overlap, is rrrmc_overlaps' and is never counted.  RRRMC_XOV_NO_LDS_HIST=1, read at the call, replaces
 *                         the per-workgroup LDS histogram by one global atomic per pair
 * Both serve every context rrrmc_snapshot_store serves (GraphQuant, the ensembles and the pattern machines with the whole N = Nk*M
 * configuration), multi-device ones included (the packed rows are gathered on the first shard's device through the host), and neither
 * disturbs a run.  npairs = 0 returns RRRMC_OK and writes nothing.  RRRMC_ERR_INVALID_ARG: npairs < 0, a NULL pointer with npairs > 0,
 * an empty or out-of-range slot, rows outside the context, npairs > 65535, npairs * nA * nB > 2^26 (256 MiB of results). */
RRRMC_API int32_t rrrmc_cross_overlaps(rrrmc_ctx *ctx, int64_t npairs, const int32_t *slotA, const int32_t *slotB, int64_t a0, int64_t nA,
                                       int64_t b0, int64_t nB, int32_t *q_out);
RRRMC_API int32_t rrrmc_overlap_hist(rrrmc_ctx *ctx, int64_t npairs, const int32_t *slotA, const int32_t *slotB, int64_t *hist_out);
/* Replica exchange (parallel tempering) between two contexts of ONE graph on one device: a temperature is a context, a ladder of T
 * temperatures is T contexts, and ladder r is replica r of each of them.  For every replica r, with Ea[r], Eb[r] the energies of the two
 * live configurations in the model's own units as Float64 (what rrrmc_energy / rrrmc_energy_f64 report; RRRMC_MODEL_SPARSE_LEVELS through
 * rrrmc_set_level_scale),
 *     dB = beta_a - beta_b;  dE = Ea[r] - Eb[r];  x = dB * dE          (three roundings, no fused multiply-add)
 *     the two configurations are swapped  iff  x >= 0  or  u < det_exp(x)
 * where u = ((w[0] << 32 | w[1]) >> 11) * 2^-53 and w = Philox4x32-10 with key (lo32(seed), hi32(seed)) and counter (lo32(round),
 * hi32(round), replica0 + r, 14): the EXCHANGE stream, a function of (seed, round, global replica id) only.  The Float64 models
 * recompute energy(X, C); the integer models take the exact tracked energy of a standardMC call when nothing has touched the
 * configuration since, and recompute otherwise.  So an exchange is a pure function of the two configurations, the two betas, seed and round.
 *   rrrmc_exchange_async    queues the exchange behind everything queued on BOTH contexts' streams, and everything queued on either
 *                           later runs behind it (events between the two streams; no host synchronisation).  Afterwards both contexts
 *                           are in the state rrrmc_set_spins leaves: no live run, caches stale, rrrmc_tracked_energy(_f64) answers
 *                           RRRMC_ERR_STATE until the next sampling call; rrrmc_fetch_results still returns the last call's samples
 *                           (they belong to the temperature, not to the walker) and rrrmc_iterations_done is unchanged
 *   rrrmc_exchange_results  waits for the last exchange whose FIRST argument was `a` and returns swapped_out[R] (1 = swapped), their
 *                           count, and the energies Ea_out[R], Eb_out[R] the verdicts were taken from (before the swap).  Any pointer
 *                           may be NULL.  RRRMC_ERR_STATE when there was no such exchange
 * Covered: RRRMC_MODEL_SPARSE_PM1 (the big-N and colour-sweep contexts included), SPARSE_LEVELS, SPARSE_F64, SK_NORMAL, SK_BINARY.
 * The library does NOT compare the two contexts' disorder: the caller states that both hold the same graph (the Python driver builds
 * every context from one graph object).  Two handles made by rrrmc_ctx_create_multi over the same device list exchange shard by shard.
 * Refusals leave both contexts untouched and set rrrmc_last_error(a): RRRMC_ERR_INVALID_ARG for a NULL handle, a == b or a beta that is
 * not finite; RRRMC_ERR_STATE when a context has no graph or no configuration, or model, N, K, R or replica0 differ;
 * RRRMC_ERR_UNSUPPORTED for every other model (GraphQuant and the ensembles carry beta inside the Hamiltonian; the message names the
 * model), for contexts on different devices, for unequal device lists, and for more than 65535 replica groups (the replicas that
 * share a word of the native spin layout) per context or shard. */
RRRMC_API int32_t rrrmc_exchange_async(rrrmc_ctx *a, rrrmc_ctx *b, double beta_a, double beta_b, uint64_t seed, uint64_t round);
RRRMC_API int32_t rrrmc_exchange_results(rrrmc_ctx *a, uint8_t *swapped_out, int64_t *nswapped_out, double *Ea_out, double *Eb_out);
/* GraphQuant observables of the live configuration of every replica (RRRMC_MODEL_QUANT_RRG):
 *   Qenergy_out[R]   Qenergy(X, C)            (src/graphs/QT.jl:253-268)
 *   tmag_out[R]      transverse_mag(X0, C, beta) (QT.jl:113-122)
 *   ovs_out[R * (M/2)] overlaps(X)            (QT.jl:213-251)
 * Any output may be NULL.  The integer sums run on the device; the Float64 tail follows the reference's operation order. */
RRRMC_API int32_t rrrmc_quant_observables(rrrmc_ctx *ctx, double beta, double Gamma, double *Qenergy_out, double *tmag_out,
                                          double *ovs_out);
/* Renergies(X) (QT.jl:201-211) of a context made by rrrmc_ctx_create_quant_pattern: out[R * M] = energy(X1[k], C1[k]) of every slice of
 * the live configuration — the training errors (GraphPercLinear: in its units of 2 / sqrt(Nk)) — recomputed from the configuration on the
 * device.  Read-only: a run the context continues is not disturbed. */
RRRMC_API int32_t rrrmc_quant_renergies(rrrmc_ctx *ctx, double *out);
/* Which build of the sampler kernels the last rrrmc_rrr_mc_async / rrrmc_standard_mc_async call on a context made by
 * rrrmc_ctx_create_quant_pattern ran (the first shard of a multi-device context): 0 = one thread per replica, 1 = one wavefront per replica
 * with the slices' Stabilities in HBM/L2, 2 = one wavefront per replica with them staged in LDS.  Chosen by the rule of the other GraphQuants:
 * up to 2048 replicas (RRRMC_QUANT_WAVE_MAX_R) run a wave build unless RRRMC_QUANT_NO_WAVE=1, with LDS staging when the state fits 160 KB
 * unless RRRMC_QUANT_NO_LDS=1.  The builds give the same bits, and any of them continues a run another began (rrrmc_set_resume). */
RRRMC_API int32_t rrrmc_quant_pattern_build(rrrmc_ctx *ctx, int32_t *build_out);

/* ---- host-side graph constructors (setup, not hot): the disorder formats of SURVEY.md §8 a7/a8 ---- */
/* gen_RRG (src/graphs/RRG.jl:26-69): A_out[N*K] 0-based, rows ascending. GRAPH stream of `seed`. */
RRRMC_API int32_t rrrmc_gen_rrg(int64_t N, int64_t K, uint64_t seed, int32_t *A_out);
/* gen_EA (src/graphs/EA.jl:24-43): periodic L^D lattice, A_out[L^D * 2D]. */
RRRMC_API int32_t rrrmc_gen_ea(int64_t L, int64_t D, int32_t *A_out);
/* gen_J with LEV = (-1, 1) (src/graphs/RRG.jl:71-96, :154-156): J_out[N*K]. COUPLING stream. */
RRRMC_API int32_t rrrmc_gen_couplings_pm1(int64_t N, int64_t K, const int32_t *A, uint64_t seed, int8_t *J_out);

#ifdef __cplusplus
}
#endif
#endif /* RRRMC_HIP_H */
