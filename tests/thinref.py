"""ef_map_thin / ef_map_thin_select restated in numpy from include/ef_hip.h alone (the section "Thin the map"), shared by test_thin_host.py
and test_gpu_thin.py.  The cell is queryref.cells_of (the f32 product with f32(1) / f32(cell), floored, clamped to +-2^20), the participants
are selectref.select_mask's rows with a finite position, and the representative of a cell is the maximum under (primary descending, row
ascending) with -0 = +0 and every NaN = -inf.  One np.unique over the cell triples and one lexsort: no loop over cells."""
import numpy as np

import selectref as sr
from queryref import cells_of

F = np.float32
KEEP_MAX_CONF, KEEP_NEWEST, KEEP_FIRST = 0, 1, 2
ROWS_REMOVED, ROWS_REPRESENTATIVES = 0, 1


def primary(surfels, keep):
    """the primary per row as float32 VALUES made totally ordered: NaN -> -inf, -0 -> +0"""
    S = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    if keep == KEEP_MAX_CONF:
        v = S[:, 3].copy()
    elif keep == KEEP_NEWEST:
        v = S[:, 7].copy()
    else:
        assert keep == KEEP_FIRST, keep
        v = np.zeros(len(S), F)
    v[np.isnan(v)] = -np.inf
    v[v == 0] = 0          # (-0 == 0 is true: both become +0)
    return v


def participants(surfels, among=None, probs=None):
    S = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    part = np.isfinite(S[:, :3]).all(1)
    if among is not None:
        part &= sr.select_mask(S, among, probs)
    return part


def thin(surfels, cell, keep=KEEP_MAX_CONF, among=None, probs=None):
    """dict: part / rep / removed (boolean per row), rows_removed / rows_rep (ascending uint32), result (ef_thin_result as a dict), kept
    (boolean per row: what ef_map_thin leaves, in order)"""
    S = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    n = len(S)
    part = participants(S, among, probs)
    idx = np.nonzero(part)[0]
    rep = np.zeros(n, bool)
    if len(idx):
        with np.errstate(invalid="ignore", over="ignore"):
            cells = cells_of(S[idx, :3], cell)
        _, cid = np.unique(cells, axis=0, return_inverse=True)
        cid = np.asarray(cid).reshape(-1)
        v = primary(S[idx], keep).astype(np.float64)      # (exact; the negation below is exact too)
        order = np.lexsort((idx, -v, cid))                # by cell, then primary descending, then row ascending
        first = np.ones(len(order), bool)
        first[1:] = cid[order][1:] != cid[order][:-1]
        rep[idx[order[first]]] = True
    removed = part & ~rep
    res = dict(participants=int(part.sum()), cells=int(rep.sum()), removed=int(removed.sum()), count_after=n - int(removed.sum()))
    return dict(part=part, rep=rep, removed=removed, rows_removed=np.nonzero(removed)[0].astype(np.uint32),
                rows_rep=np.nonzero(rep)[0].astype(np.uint32), result=res, kept=~removed)
