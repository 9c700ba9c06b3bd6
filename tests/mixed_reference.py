"""Plain-Python restatement of GraphMixed (src/graphs/Mixed.jl:15-61): two or more graphs on one set of spins,

    energy(X, C)          = sum(energy(x, C) for x in X.graphs)              (:33-36)
    delta_energy(X, C, i) = sum(delta_energy(x, C, i) for x in X.graphs)     (:38-40)
    update_cache!(X, C, i) = every component's, in order                    (:42-47)

Julia's ``sum`` over a generator folds from the left and starts with the first element: ((d1 + d2) + d3) ...  The components are the slice
objects of re_reference / perc_reference / comm_reference / comm_qu_reference / sat_reference / sparse_slice_reference and the xentr
restatement (``energy(s)``, which also builds the cache, ``delta(s, i)``, ``flip_update(s, i)`` after the flip of ``s[i]``), so a ``Mixed``
has their interface too and is usable as the ``g`` of ``add_fields_reference.AddFields``, and under its ``standard_mc`` as
``AddFields(h, mixed, sub=True)`` (GraphAddSubFields' energy and delta_energy are g's own)."""
import numpy as np

import add_fields_reference as AF
import re_reference as RE
import sparse_slice_reference as SSR
import xentr_reference as XR


class Mixed:
    def __init__(self, parts):
        self.parts = list(parts)
        if len(self.parts) < 2:
            raise ValueError("at least 2 base graphs needed")               # Mixed.jl:22
        self.skn_swaps = self.spf_undos = 0                                  # instrumentation: the undo paths of the two caches that follow every flip

    def energies(self, s):
        return [p.energy(s) for p in self.parts]

    def energy(self, s):
        es = self.energies(s)
        E = es[0]
        for e in es[1:]:
            E = E + e
        return E

    def delta(self, s, i):
        d = self.parts[0].delta(s, i)
        for p in self.parts[1:]:
            d = d + p.delta(s, i)
        return d

    def flip_update(self, s, i):
        for p in self.parts:
            if isinstance(p, RE.SliceSKN) and getattr(p, "move_last", None) == i:
                self.skn_swaps += 1
            if isinstance(p, SSR.SliceSparseF64) and p.move_last == i:
                self.spf_undos += 1
            p.flip_update(s, i)


def part_of(g, N):
    """the restatement of one component of a product GraphMixed (None: GraphEmpty)"""
    if g is None:
        return RE.SliceEmpty(N)
    name = type(g).__name__
    if name in ("GraphRRGNormal", "GraphEANormal", "_SparseF64Graph"):
        return SSR.SliceSparseF64(g.A, g.J)
    if name in ("GraphRRG", "GraphEA"):                                       # ±J as ±1.0
        return SSR.SliceSparseF64(g.A, np.asarray(g.J, np.float64))
    if name == "GraphPercXEntr":
        return XR.PercXEntrRef(g.patterns(), Hs=g.Hs)
    return AF.slice_of(g)


def reference_of(X):
    """the restatement of a product GraphMixed, or of a GraphAddFields / GraphAddSubFields over one, with fresh components"""
    if type(X).__name__ == "GraphMixed":
        return Mixed([part_of(g, X.N) for g in X.graphs])
    return AF.AddFields(X.fields, reference_of(X.X1), type(X).__name__ == "GraphAddSubFields")


def as_chain(X):
    """a restatement that add_fields_reference.standard_mc drives: the stand-alone mix as GraphAddSubFields over zero fields (its energy and
    delta_energy are the mix's own)"""
    ref = reference_of(X)
    return AF.AddFields([0.0] * X.N, ref, True) if isinstance(ref, Mixed) else ref
