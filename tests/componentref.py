"""The connected components of include/ef_hip.h ("Connected components of the map") restated in numpy from the header alone: the node rule, an
exhaustive f32 d2 matrix with the header's bracketing, a sequential union-find over its edges, the smallest row of every component as its
label, sizes, verdicts, lists and the result.  No grid, no index, no scipy.  Every output is an integer: the device must equal it exactly."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
REJECTED, ACCEPTED = 0, 1
DEFAULTS = dict(radius=0.03, min_conf=-1.0, min_size=50, max_size=0)


def participants(S, among=None):
    """among: a bool mask of the selected rows, or None"""
    with np.errstate(invalid="ignore"):
        fin = (np.abs(S[:, :3].astype(F)) <= np.finfo(F).max).all(1)
    return fin if among is None else fin & np.asarray(among, bool)


def nodes(S, among=None, min_conf=-1.0):
    """participants whose confidence passes conf > min_conf (a NaN confidence compares false)"""
    with np.errstate(invalid="ignore"):
        return participants(S, among) & (S[:, 3].astype(F) > F(min_conf))


def edges(S, node, radius, chunk=512):
    """[m, 2] int64 (s, t) with s > t: every pair of distinct nodes with d2(p_s, p_t) <= r2, d2 = ((dx * dx + dy * dy) + dz * dz) in f32"""
    S = np.ascontiguousarray(S, F)
    n = len(S)
    r = F(radius)
    r2 = F(r * r)
    px, py, pz = S[:, 0], S[:, 1], S[:, 2]
    rows = np.arange(n)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, chunk):
            q = slice(a, min(a + chunk, n))
            dx = px[q, None] - px[None, :]
            dy = py[q, None] - py[None, :]
            dz = pz[q, None] - pz[None, :]
            d2 = ((dx * dx + dy * dy) + dz * dz)
            assert d2.dtype == F
            hit = (d2 <= r2) & node[q, None] & node[None, :] & (rows[q, None] > rows[None, :])
            s, t = np.nonzero(hit)
            out.append(np.stack([s + a, t], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def union_find(n, pairs):
    """the sequential union-find: parent [n] after every pair was united, fully compressed (parent[x] = the root of x)"""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for s, t in pairs.tolist() if isinstance(pairs, np.ndarray) else pairs:
        a, b = find(s), find(t)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], np.int64)


def labels_of(n, node, pairs):
    """(label uint32, size uint32): the smallest row of each node's component, its number of nodes; NONE and 0 for a row that is no node"""
    root = union_find(n, pairs)
    low = np.full(n, n, np.int64)
    np.minimum.at(low, root, np.arange(n))                 # the smallest row of every set (the root is it already; this does not rely on that)
    lab = low[root]
    members = np.bincount(lab[node], minlength=max(n, 1))
    label = np.where(node, lab, NONE).astype(np.uint32)
    size = np.where(node, members[np.where(node, lab, 0)], 0).astype(np.uint32) if n else np.zeros(0, np.uint32)
    return label, size


def components(S, among=None, pairs=None, **kw):
    """everything the header defines for one call.  pairs: edges(S, node, radius) when the caller has it already"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    node = nodes(S, among, p["min_conf"])
    if pairs is None:
        pairs = edges(S, node, p["radius"])
    label, size = labels_of(n, node, pairs)
    lo, hi = np.uint32(p["min_size"]), np.uint32(p["max_size"])
    rejected = node & ((size < lo) | ((hi != 0) & (size > hi)))
    accepted = node & ~rejected
    is_root = node & (label == np.arange(n, dtype=np.uint32))
    res = dict(nodes=int(node.sum()), components=int(is_root.sum()), largest=int(size.max()) if n else 0, rejected_rows=int(rejected.sum()),
               rejected_components=int((is_root & rejected).sum()), count_after=n - int(rejected.sum()), status=0)
    return dict(label=label, size=size, node=node, pairs=pairs, rejected=np.nonzero(rejected)[0].astype(np.uint32),
                accepted=np.nonzero(accepted)[0].astype(np.uint32), result=res)


def same_partition(label_a, label_b, perm):
    """row i of map A is row perm[i] of map B: the two labelings give the same partition (and the same non-nodes)"""
    la, lb = np.asarray(label_a, np.int64), np.asarray(label_b, np.int64)[perm]
    if not np.array_equal(la == NONE, lb == NONE):
        return False
    keep = la != NONE
    pairs = np.unique(np.stack([la[keep], lb[keep]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
