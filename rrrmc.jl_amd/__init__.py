"""MI355X-native Ising Monte Carlo sweep engine behind RRRMC.jl's graph / sampler API.

Host-side mirror (Python, since Julia is not available in this image) of the reference interface for
the hot path: ``Config`` (src/Interface.jl:21-29), ``GraphRRG`` (src/graphs/RRG.jl:116-162), ``GraphEA``
(src/graphs/EA.jl:138-193) and ``standardMC`` (src/RRRMC.jl:81-127).  All computation happens in the
gfx950 library ``lib/librrrmc_hip.so`` through the C ABI of ``include/rrrmc_hip.h``.
"""
from ._lib import RRRMCError, SYMBOLS, lib, pinned_empty  # noqa: F401
from .graphs import Config, GraphCommQu, GraphCommQuLE, GraphCommQuRE, GraphQCommQuT, GraphCommReLU, GraphCommReLULE, GraphCommReLURE, GraphCommStep, GraphCommStepLE, GraphCommStepRE, Graph0LE, Graph0RE, GraphEA, GraphEANormal, GraphEANormalDiscretized, GraphLocalEntropy, GraphPercLinear, GraphPercLinearLE, GraphPercLinearRE, GraphPercStep, GraphPercStepLE, GraphPercStepRE, GraphQCommReLUT, GraphQCommStepT, GraphQEAT, GraphQPercLinearT, GraphQPercStepT, GraphQSKNormalT, GraphQSKT, GraphQuant, Qenergy, Renergies, overlaps, transverse_mag, GraphRRG, GraphRRGNormal, GraphRRGNormalDiscretized, GraphRobustEnsemble, GraphSAT, GraphSATLE, GraphSATRE, GraphSK, GraphSKLE, GraphSKNormal, GraphSKRE, LEenergies, REenergies, all_delta_e, cenergy, checkerboard_coloring, distances, getN, level_units, neighbors  # noqa: F401
from .engine import EnergyProbe, Engine, bklMC, energy, extremal_opt, rrrMC, standardMC, wtmMC  # noqa: F401
from .observables import SnapshotLog, bitmatrix_chunks, get_ts_range, log_range, parseovs, parsets  # noqa: F401
from .sharding import gather_replica_major, shard_bounds  # noqa: F401

__all__ = ["Config", "GraphRRG", "GraphEA", "GraphSKNormal", "GraphSK", "GraphRRGNormal", "GraphEANormal", "GraphRRGNormalDiscretized", "GraphEANormalDiscretized", "GraphQuant", "GraphQSKT", "GraphQSKNormalT", "GraphQEAT", "GraphQPercStepT", "GraphQPercLinearT", "GraphQCommStepT", "GraphQCommReLUT", "GraphQCommQuT", "Renergies", "Qenergy", "transverse_mag", "overlaps", "GraphRobustEnsemble", "GraphSKRE", "Graph0RE", "REenergies", "GraphLocalEntropy", "GraphSKLE", "Graph0LE", "LEenergies", "cenergy", "distances", "GraphPercStep", "GraphPercLinear", "GraphPercStepRE", "GraphPercLinearRE", "GraphPercStepLE", "GraphPercLinearLE", "GraphCommStep", "GraphCommReLU", "GraphCommQu", "GraphCommStepRE", "GraphCommReLURE", "GraphCommQuRE", "GraphCommStepLE", "GraphCommReLULE", "GraphCommQuLE", "GraphSAT", "GraphSATRE", "GraphSATLE", "rrrMC", "bklMC", "wtmMC", "extremal_opt", "checkerboard_coloring", "Engine", "EnergyProbe", "energy", "standardMC", "RRRMCError", "getN", "neighbors", "all_delta_e", "level_units",
           "shard_bounds", "gather_replica_major", "pinned_empty", "SnapshotLog", "parseovs", "parsets", "log_range", "get_ts_range", "bitmatrix_chunks"]
