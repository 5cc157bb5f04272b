"""References for the device builders' BINARY trees, the collapse's cost table and the collapse itself (nx_lbvh.hip), in numpy.

TEST INFRASTRUCTURE ONLY.  No GPU, no product code: what is judged is a tree as `Context.debug_read_binary_tree` returns it (a dict:
n, prim_cost, builder, left / right / count [n - 1], parent [2n - 1], box [2n - 1, 2, 3], leaf_order [n], cost / decision / left_count /
right_count [n - 1, 7]) together with the primitive boxes it was built from and the wide nodes it was collapsed into.  Internal nodes are
0 .. n-2 (the root is 0), leaf k is node n-1+k and holds primitive leaf_order[k].

The library is compiled without contraction of a * b + c, so an expression restated in np.float32 with the kernel's order of operations
gives the kernel's bits wherever the kernel is deterministic; those checks are equalities.  Where atomics decide (node numbers) trees
are compared as nested sets, and where the kernel only has to be as good as the best candidate (the top-down SAH build) the check is
an optimality bound in float64:

  (a) check_structure      n leaves, every primitive once, links consistent, counts, every box the exact union of its children's
  (b) check_radix          the Morton radix tree, from its definition (highest differing bit of the key (code, position))
  (c) check_clustering     locally-ordered clustering, round by round
  (d) check_sah            the top-down binned SAH build: every node's split is a candidate and costs no more than the best one
  (e) check_cost_table     the SAH-DP table: each node's entries bit-exact from its children's, and every cost against a float64 DP
  (f) check_collapse       the 8-wide nodes: an exact replay of the gather, the slot assignment, the numbering and the quantisation,
                           and the float64 cost of the result against the DP's optimum

Every check raises TreeError (an AssertionError) with the first few offending nodes.  tests/test_binary_tree_reference.py judges the
checks themselves: each accepts trees built here on the CPU from the same definitions and refuses a planted defect of its kind.

Bounds (both derived, none tuned):
  SAH_SLACK = 2^-20.  The builder compares costs count_L * A(L) + count_R * A(R) computed in binary32: three subtractions, three
    products and two sums per area, a product with the count and the final sum — at most 8 roundings of 2^-24 in sequence on sums of
    positive terms, on either of the two costs compared: its pick is within (1 + 2^-24)^16 < 1 + 2^-20 of the best candidate.
  DP bound = (2 * height + 8) * 2^-24, relative.  A cost is a sum of positive terms; an entry adds one sum to its children's entries
    (and entry 0 one more for the node test), so errors grow by at most 2 roundings per level on top of the 8 of an area and its
    products at the leaves.
"""
import numpy as np

F = np.float32
SAH_BINS, SAH_SMALL, LEAF_MAX = 16, 8, 3
DEC_LEAF, DEC_INTERNAL, DEC_DISTRIBUTE = 0, 1, 2
SAH_SLACK = 2.0 ** -20


class TreeError(AssertionError):
    pass


def _fail(what, items=()):
    items = list(items)
    raise TreeError(what + (": " + "; ".join(str(x) for x in items[:4]) + (" ... %d in all" % len(items) if len(items) > 4 else "") if items else ""))


def dp_bound(height):
    return (2 * height + 8) * 2.0 ** -24


# ---- shared arithmetic ----------------------------------------------------------------------------------------------
def centres(plo, phi):
    """0.5f * (lo + hi) in binary32"""
    return (F(0.5) * (np.asarray(plo, F) + np.asarray(phi, F))).astype(F)


def half_area32(lo, hi):
    """ex * ey + ey * ez + ex * ez, every operation rounded to binary32, summed left to right (half_area / union_half_area)"""
    e = (np.asarray(hi, F) - np.asarray(lo, F)).astype(F)
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    return (((ex * ey).astype(F) + (ey * ez).astype(F)).astype(F) + (ex * ez).astype(F)).astype(F)


def half_area64(lo, hi):
    e = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 0] * e[..., 2]


def levels_of(T):
    """internal nodes by depth, from the root; raises unless the links form one tree over all 2n - 1 nodes"""
    n = T["n"]
    left, right, parent = np.asarray(T["left"], np.int64), np.asarray(T["right"], np.int64), np.asarray(T["parent"], np.int64)
    kids = np.concatenate([left, right])
    if kids.min() < 1 or kids.max() > 2 * n - 2 or len(np.unique(kids)) != 2 * n - 2:
        _fail("the children are not every node but the root exactly once")
    if parent[0] != -1:
        _fail("the root's parent is %d" % parent[0])
    inner = np.arange(n - 1)
    bad = inner[(parent[left] != inner) | (parent[right] != inner)]
    if len(bad):
        _fail("parent does not point back from a child", bad)
    levels, frontier, seen = [], np.array([0], np.int64), 0
    while len(frontier):
        if len(levels) > 2 * n:
            _fail("the links form a cycle")
        levels.append(frontier)
        seen += len(frontier)
        nxt = np.concatenate([left[frontier], right[frontier]])
        seen += int((nxt >= n - 1).sum())
        frontier = nxt[nxt < n - 1]
    if seen != 2 * n - 1:
        _fail("%d of %d nodes are reached from the root" % (seen, 2 * n - 1))
    return levels


def leaf_ranges(T, levels):
    """(first, last) leaf position under every node, bottom-up"""
    n = T["n"]
    first, last = np.zeros(2 * n - 1, np.int64), np.zeros(2 * n - 1, np.int64)
    first[n - 1:] = last[n - 1:] = np.arange(n)
    for lv in reversed(levels):
        l, r = T["left"][lv], T["right"][lv]
        first[lv] = np.minimum(first[l], first[r])
        last[lv] = np.maximum(last[l], last[r])
    return first, last


# ---- (a) structure ----------------------------------------------------------------------------------------------------
def check_structure(T, plo, phi, loose_ok=None):
    """-> (levels, height).  Every internal box must EQUAL the union of its two children's boxes and every leaf box its primitive's: min
    and max do not round, so a parent fitted from a child's stale box shows (equal as numbers: of two zeros fmin may return either).
    loose_ok: internal nodes allowed to be wider than that union (the children of a top-down node that nothing separates carry the
    node's own box — check_sah names them and checks that they do); they must still contain it."""
    n = T["n"]
    plo, phi = np.asarray(plo, F), np.asarray(phi, F)
    if n != len(plo) or n < 2:
        _fail("a tree over %d primitives for %d boxes" % (n, len(plo)))
    for k, size in (("left", n - 1), ("right", n - 1), ("count", n - 1), ("parent", 2 * n - 1), ("box", 2 * n - 1), ("leaf_order", n)):
        if len(T[k]) != size:
            _fail("%s has %d entries, not %d" % (k, len(T[k]), size))
    order = np.asarray(T["leaf_order"], np.int64)
    if not np.array_equal(np.sort(order), np.arange(n)):
        _fail("leaf_order is not a permutation of the primitives")
    levels = levels_of(T)
    left, right = np.asarray(T["left"], np.int64), np.asarray(T["right"], np.int64)
    below = np.ones(2 * n - 1, np.int64)
    for lv in reversed(levels):
        below[lv] = below[left[lv]] + below[right[lv]]
    bad = np.nonzero(below[:n - 1] != np.asarray(T["count"], np.int64))[0]
    if len(bad):
        _fail("count is not the number of leaves below", ["node %d: %d for %d" % (x, T["count"][x], below[x]) for x in bad])
    box = np.asarray(T["box"], F)
    if not np.all(np.isfinite(box)):
        _fail("a box is not finite")
    leaf = box[n - 1:]
    bad = np.nonzero(np.any(leaf[:, 0] != plo[order], axis=1) | np.any(leaf[:, 1] != phi[order], axis=1))[0]
    if len(bad):
        _fail("a leaf's box is not its primitive's", ["leaf %d (primitive %d)" % (k, order[k]) for k in bad])
    ulo = np.minimum(box[left, 0], box[right, 0])
    uhi = np.maximum(box[left, 1], box[right, 1])
    exact = np.all(box[:n - 1, 0] == ulo, axis=1) & np.all(box[:n - 1, 1] == uhi, axis=1)
    holds = np.all(box[:n - 1, 0] <= ulo, axis=1) & np.all(box[:n - 1, 1] >= uhi, axis=1)
    ok = exact if loose_ok is None else np.where(np.asarray(loose_ok, bool), holds, exact)
    bad = np.nonzero(~ok)[0]
    if len(bad):
        _fail("an internal box is not the union of its children's", ["node %d: [%s, %s] for [%s, %s]" % (x, box[x, 0], box[x, 1], ulo[x], uhi[x]) for x in bad])
    return levels, len(levels)


# ---- Morton order (radix tree and clustering start from it) -----------------------------------------------------------
def _spread21(v):
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for sh, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(mask)
    return x


def morton_codes(plo, phi):
    """morton_kernel: 21 bits per axis of the box centre within the centroid bounds, all in binary32"""
    c = centres(plo, phi)
    lo, hi = c.min(0), c.max(0)
    ext = (hi - lo).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ext > 0, (F(2097151.0) / ext).astype(F), F(0.0)).astype(F)
    f = ((c - lo).astype(F) * inv).astype(F)
    q = np.minimum(np.maximum(f, F(0.0)), F(2097151.0)).astype(np.uint32)
    return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])


def morton_order(plo, phi):
    """(sorted codes, order): stable by (code, primitive index), what a stable radix sort of (code, index) pairs gives"""
    codes = morton_codes(plo, phi)
    order = np.argsort(codes, kind="stable")
    return codes[order], order


# ---- (b) radix tree ---------------------------------------------------------------------------------------------------
def radix_splits(codes_sorted, tie_by_index=True):
    """{(first, last): split} of the radix tree over the sorted keys, from its DEFINITION: the node over [first, last] divides at the
    highest bit in which key[first] and key[last] differ (the positions left of `split + 1` have it clear); the key is the code
    followed by the position, so equal codes divide by the bits of their positions.  tie_by_index=False is the planted defect: a run
    of equal codes halved."""
    keys = [(int(c) << 32) | i for i, c in enumerate(codes_sorted)]
    out, todo = {}, [(0, len(keys) - 1)]
    while todo:
        lo, hi = todo.pop()
        if lo == hi:
            continue
        if not tie_by_index and codes_sorted[lo] == codes_sorted[hi]:
            split = (lo + hi) // 2
        else:
            bit = (keys[lo] ^ keys[hi]).bit_length() - 1
            a, b = lo, hi  # keys[a] has the bit clear, keys[b] set; the prefix above it is shared, so the bit is monotone over the range
            while b - a > 1:
                m = (a + b) // 2
                if keys[m] >> bit & 1:
                    b = m
                else:
                    a = m
            split = a
        out[(lo, hi)] = split
        todo += [(lo, split), (split + 1, hi)]
    return out


def check_radix(T, plo, phi, levels=None):
    n = T["n"]
    codes, order = morton_order(plo, phi)
    if not np.array_equal(np.asarray(T["leaf_order"], np.int64), order):
        _fail("leaf_order is not the stable order of the Morton codes", np.nonzero(np.asarray(T["leaf_order"], np.int64) != order)[0])
    levels = levels_of(T) if levels is None else levels
    first, last = leaf_ranges(T, levels)
    want = radix_splits(codes)
    got = {(int(first[x]), int(last[x])): int(last[T["left"][x]]) for x in range(n - 1)}
    if got != want:
        wrong = [("range %s splits after %s, the definition after %s" % (k, got[k], want.get(k, "nothing: no such node"))) for k in sorted(got) if got[k] != want.get(k)]
        _fail("not the radix tree of the sorted keys", wrong or ["ranges missing: %s" % sorted(set(want) - set(got))[:4]])


# ---- (c) clustering ---------------------------------------------------------------------------------------------------
def clustering_build(plo, phi, radius, defect=None):
    """Locally-ordered clustering as nx_lbvh.hip 4b runs it: the sorted primitives are clusters; every round each cluster picks, among
    the up to `radius` neighbours on either side, the one with the smallest union_half_area (binary32), ties broken on the pair (smaller
    position, then larger); pairs that picked each other merge (left = the earlier), survivors keep their order.  Node numbers: downwards
    from n - 2 in merge order, so the last merge is node 0.  defect="non_mutual": in the first round that has such pairs, pairs merge of which
    only one picked the other."""
    plo, phi = np.asarray(plo, F), np.asarray(phi, F)
    n = len(plo)
    _, order = morton_order(plo, phi)
    left, right, count = (np.zeros(n - 1, np.int32) for _ in range(3))
    parent = np.full(2 * n - 1, -1, np.int32)
    box = np.zeros((2 * n - 1, 2, 3), F)
    box[n - 1:, 0], box[n - 1:, 1] = plo[order], phi[order]
    size = np.ones(2 * n - 1, np.int64)
    cluster = np.arange(n - 1, 2 * n - 1)
    made = 0
    planted = defect != "non_mutual"
    while len(cluster) > 1:
        m = len(cluster)
        lo, hi = box[cluster, 0], box[cluster, 1]
        best = np.full(m, np.inf, F)
        pick = np.full(m, -1, np.int64)
        blo, bhi = np.zeros(m, np.int64), np.zeros(m, np.int64)
        idx = np.arange(m)
        for d in [x for x in range(-radius, radius + 1) if x]:
            j = idx + d
            ok = (j >= 0) & (j < m)
            jj = np.clip(j, 0, m - 1)
            a = half_area32(np.minimum(lo, lo[jj]), np.maximum(hi, hi[jj]))
            plo_, phi_ = np.minimum(idx, jj), np.maximum(idx, jj)
            better = ok & ((pick < 0) | (a < best) | ((a == best) & ((plo_ < blo) | ((plo_ == blo) & (phi_ < bhi)))))
            best, pick, blo, bhi = np.where(better, a, best), np.where(better, jj, pick), np.where(better, plo_, blo), np.where(better, phi_, bhi)
        mutual = pick[pick] == idx
        if not planted:
            for i in np.nonzero(~mutual & ~mutual[pick])[0]:  # i picked j, j picked someone else, neither merges this round: merge them
                j = int(pick[i])
                if not mutual[i] and not mutual[j]:
                    pick[j] = i
                    mutual[[i, j]] = True
                    planted = True
        keep = np.ones(m, bool)
        merged = cluster.copy()
        for i in np.nonzero(mutual & (idx < pick))[0]:
            j = pick[i]
            a, b = cluster[i], cluster[j]
            node = n - 2 - made
            made += 1
            left[node], right[node] = a, b
            parent[a] = parent[b] = node
            box[node, 0], box[node, 1] = np.minimum(box[a, 0], box[b, 0]), np.maximum(box[a, 1], box[b, 1])
            size[node] = size[a] + size[b]
            count[node] = size[node]
            merged[i] = node
            keep[j] = False
        if keep.all():
            _fail("a clustering round merged nothing")
        cluster = merged[keep]
    parent[0] = -1
    return {"n": n, "left": left, "right": right, "parent": parent, "count": count, "box": box, "leaf_order": order.astype(np.uint32)}


def nested_sets(T, names):
    """the tree as nested (left, right) pairs of primitives, each distinct subtree a number from the shared table `names`; -> the root's"""
    n = T["n"]
    sig = np.zeros(2 * n - 1, np.int64)
    order = np.asarray(T["leaf_order"], np.int64)
    for k in range(n):
        sig[n - 1 + k] = names.setdefault(("p", int(order[k])), len(names))
    for lv in reversed(levels_of(T)):
        for x in lv:
            sig[x] = names.setdefault((int(sig[T["left"][x]]), int(sig[T["right"][x]])), len(names))
    return sig


def check_clustering(T, plo, phi, radius):
    want = clustering_build(plo, phi, radius)
    names = {}
    a, b = nested_sets(want, names), nested_sets(T, names)
    if a[0] != b[0]:
        known = set(a.tolist())
        odd = [x for x in range(T["n"] - 1) if int(b[x]) not in known]
        _fail("not the tree the clustering rounds give (radius %d)" % radius, ["node %d (%d primitives) is no subtree of it" % (x, T["count"][x]) for x in sorted(odd, key=lambda x: T["count"][x])])


# ---- (d) top-down SAH ---------------------------------------------------------------------------------------------------
def sah_bin(c, lo, hi):
    """the bin of a centroid coordinate (sah_bin): binary32 throughout"""
    scale = F(F(SAH_BINS) / F(hi - lo))
    f = ((np.asarray(c, F) - F(lo)).astype(F) * scale).astype(F)
    return np.where(f >= 0, np.minimum(f, F(SAH_BINS - 1)), F(0.0)).astype(np.int64)


def _cut_costs(lo, hi, key, axis=0):
    """Sorted by `key` (stable) along `axis`: count_L * A(L) + count_R * A(R) in float64 for every cut of the sorted order, and whether the
    cut lies between two DIFFERENT keys.  lo / hi [..., m, 3], key [..., m] -> (cost [..., m - 1], distinct [..., m - 1]); cut j leaves j + 1 left"""
    p = np.argsort(key, axis=-1, kind="stable")
    k = np.take_along_axis(key, p, -1)
    L, H = np.take_along_axis(lo, p[..., None], -2), np.take_along_axis(hi, p[..., None], -2)
    m = key.shape[-1]
    pl, ph = np.minimum.accumulate(L, -2), np.maximum.accumulate(H, -2)
    sl, sh = np.minimum.accumulate(L[..., ::-1, :], -2)[..., ::-1, :], np.maximum.accumulate(H[..., ::-1, :], -2)[..., ::-1, :]
    left = np.arange(1, m)
    cost = left * half_area64(pl[..., :-1, :], ph[..., :-1, :]) + (m - left) * half_area64(sl[..., 1:, :], sh[..., 1:, :])
    return cost, k[..., 1:] > k[..., :-1]


def check_sah(T, plo, phi, levels=None):
    """Node by node on the tree itself.  -> (loose_ok for check_structure, the largest cost(split) / cost(best candidate) - 1 seen)."""
    n = T["n"]
    plo, phi = np.asarray(plo, F), np.asarray(phi, F)
    levels = levels_of(T) if levels is None else levels
    first, last = leaf_ranges(T, levels)
    left, right, count = np.asarray(T["left"], np.int64), np.asarray(T["right"], np.int64), np.asarray(T["count"], np.int64)
    inner = np.arange(n - 1)
    bad = inner[(last[inner] + 1 - first[inner] != count) | (first[left] != first[inner]) | (last[left] + 1 != first[right]) | (last[right] != last[inner])]
    if len(bad):
        _fail("top-down SAH: a node's leaves are not one range, left part first", bad)
    order = np.asarray(T["leaf_order"], np.int64)
    c_s = centres(plo[order], phi[order])  # by leaf position
    lo64, hi64 = plo[order].astype(np.float64), phi[order].astype(np.float64)
    box = np.asarray(T["box"], F)
    kl = last[left] + 1 - first[inner]  # primitives on the left
    loose = np.zeros(n - 1, bool)
    worst, fails = 0.0, []

    def judge(x, cnt, k, cost, best):
        nonlocal worst
        excess = cost / best - 1.0 if best > 0 else (0.0 if cost == 0 else np.inf)
        worst = max(worst, excess)
        if excess > SAH_SLACK:
            fails.append("node %d (%d primitives): split %d : %d costs %.9g, the best candidate %.9g (%.3g above)" % (x, cnt, k, cnt - k, cost, best, excess))

    # nodes of 2 .. 8 primitives, all nodes of one size at once
    for cnt in range(2, SAH_SMALL + 1):
        xs = inner[count == cnt]
        if not len(xs):
            continue
        at = first[xs][:, None] + np.arange(cnt)
        c, lo, hi, k = c_s[at], lo64[at], hi64[at], kl[xs]
        is_left = np.arange(cnt) < k[:, None]
        cl, cr = np.where(is_left[..., None], c, -np.inf).max(1), np.where(is_left[..., None], np.inf, c).min(1)
        separated = np.any(cl <= cr, axis=1)
        best = np.full(len(xs), np.inf)
        for ax in range(3):
            cost, distinct = _cut_costs(lo, hi, c[:, :, ax])
            best = np.minimum(best, np.where(distinct, cost, np.inf).min(1))
        own = _cut_costs(lo, hi, np.broadcast_to(np.arange(cnt), (len(xs), cnt)))[0][np.arange(len(xs)), k - 1]
        for i, x in enumerate(xs):
            if np.isfinite(best[i]):
                if not separated[i]:
                    fails.append("node %d (%d primitives): its two parts are separated along no axis" % (x, cnt))
                else:
                    judge(x, cnt, k[i], own[i], best[i])
            elif k[i] != cnt // 2:
                fails.append("node %d (%d primitives, centroids coincide): split %d : %d, not in half" % (x, cnt, k[i], cnt - k[i]))

    # larger nodes, from the root down: a split by position hands its centroid bounds to its children
    inherits = {}
    for lv in levels:
        for x in lv[count[lv] > SAH_SMALL]:
            x = int(x)
            a, cnt, k = int(first[x]), int(count[x]), int(kl[x])
            c, lo, hi = c_s[a:a + cnt], lo64[a:a + cnt], hi64[a:a + cnt]
            cb = inherits.get(x) or (c.min(0), c.max(0))
            best, is_candidate = np.inf, False
            for ax in range(3):
                if not cb[0][ax] < cb[1][ax]:
                    continue
                bins = sah_bin(c[:, ax], cb[0][ax], cb[1][ax])
                is_candidate |= bool(bins[:k].max() < bins[k:].min())
                cost, distinct = _cut_costs(lo, hi, bins)
                best = min(best, cost[distinct].min()) if distinct.any() else best
            if np.isfinite(best):
                if not is_candidate:
                    fails.append("node %d (%d primitives): its left part is no 'bins <= k' of a live axis" % (x, cnt))
                else:
                    judge(x, cnt, k, _cut_costs(lo, hi, np.arange(cnt))[0][k - 1], best)
                continue
            # nothing separates the centroids: halves by position, and the children carry the node's box and its centroid bounds
            if k != cnt // 2:
                fails.append("node %d (%d primitives, centroids coincide): split %d : %d, not in half" % (x, cnt, k, cnt - k))
            for ch in (int(left[x]), int(right[x])):
                if ch < n - 1:
                    loose[ch] = True
                    inherits[ch] = cb
                    if not np.array_equal(box[ch], box[x]):
                        fails.append("node %d: child %d of a split by position does not carry the node's box" % (x, ch))
    if fails:
        _fail("top-down SAH", fails)
    return loose, worst


# ---- (e) cost table -----------------------------------------------------------------------------------------------------
def _child_costs32(T, child):
    """[len(child), 7] binary32 entries as eval_of returns them: a leaf's is half_area * primCost whatever the index"""
    n = T["n"]
    child = np.asarray(child, np.int64)
    box = np.asarray(T["box"], F)
    leaf = (half_area32(box[child, 0], box[child, 1]) * F(T["prim_cost"])).astype(F)
    inner = np.asarray(T["cost"], F)[np.minimum(child, n - 2)]
    return np.where((child >= n - 1)[:, None], leaf[:, None], inner).astype(F)


def cost_entries(T, nodes):
    """cost_kernel for the internal nodes `nodes`, from the children's entries in T -> (cost f32, decision, left_count, right_count) [len, 7]"""
    nodes = np.asarray(nodes, np.int64)
    m = len(nodes)
    lc, rc = _child_costs32(T, T["left"][nodes]), _child_costs32(T, T["right"][nodes])
    box = np.asarray(T["box"], F)
    area = half_area32(box[nodes, 0], box[nodes, 1])
    prims = np.asarray(T["count"], np.int64)[nodes]
    cost, dec = np.zeros((m, 7), F), np.zeros((m, 7), np.int8)
    nl, nr = np.zeros((m, 7), np.int8), np.zeros((m, 7), np.int8)
    for i in range(7):
        j = 7 if i == 0 else i
        best, bl, br = np.full(m, F(1.0e30), F), np.zeros(m, np.int8), np.zeros(m, np.int8)
        for a in range(j):
            c = (lc[:, a] + rc[:, j - 1 - a]).astype(F)
            better = c < best
            best, bl, br = np.where(better, c, best).astype(F), np.where(better, a, bl).astype(np.int8), np.where(better, j - 1 - a, br).astype(np.int8)
        if i == 0:
            can_leaf = (prims <= LEAF_MAX) & (np.asarray(T["parent"], np.int64)[nodes] >= 0)
            leaf = ((area * prims.astype(F)).astype(F) * F(T["prim_cost"])).astype(F)
            inner = (best + (area * F(1.0)).astype(F)).astype(F)
            as_leaf = can_leaf & (leaf < inner)
            cost[:, 0] = np.where(as_leaf, leaf, inner)
            dec[:, 0] = np.where(as_leaf, DEC_LEAF, DEC_INTERNAL)
            nl[:, 0], nr[:, 0] = np.where(as_leaf, 0, bl), np.where(as_leaf, 0, br)
        else:
            better = best < cost[:, i - 1]
            cost[:, i] = np.where(better, best, cost[:, i - 1])
            dec[:, i] = np.where(better, DEC_DISTRIBUTE, dec[:, i - 1])
            nl[:, i], nr[:, i] = np.where(better, bl, nl[:, i - 1]), np.where(better, br, nr[:, i - 1])
    return cost, dec, nl, nr


def cost_table64(T, levels):
    """The recurrence above `struct Eval`, bottom-up in float64 and on its own:
    C(x, 0) = min(leaf slot if x holds at most 3 primitives and is not the root, area + min_a C(l, a) + C(r, 6 - a));
    C(x, i) = min(C(x, i - 1), min_a C(l, a) + C(r, i - 1 - a));  a single primitive: area * primCost for every i.  -> [2n - 1, 7]"""
    n = T["n"]
    box = np.asarray(T["box"], np.float64)
    area = half_area64(box[:, 0], box[:, 1])
    pc = float(F(T["prim_cost"]))
    C = np.zeros((2 * n - 1, 7))
    C[n - 1:] = (area[n - 1:] * pc)[:, None]
    for lv in reversed(levels):
        l, r = C[T["left"][lv]], C[T["right"][lv]]
        for i in range(7):
            j = 7 if i == 0 else i
            best = np.min([l[:, a] + r[:, j - 1 - a] for a in range(j)], axis=0)
            if i == 0:
                can_leaf = (np.asarray(T["count"])[lv] <= LEAF_MAX) & (lv != 0)
                C[lv, 0] = np.where(can_leaf, np.minimum(area[lv] * np.asarray(T["count"])[lv] * pc, best + area[lv]), best + area[lv])
            else:
                C[lv, i] = np.minimum(best, C[lv, i - 1])
    return C


def check_cost_table(T, levels):
    """-> (float64 table, largest relative deviation of a device cost from it)"""
    n = T["n"]
    cost, dec, nl, nr = cost_entries(T, np.arange(n - 1))
    got = np.asarray(T["cost"], F)
    bad = np.nonzero((cost.view(np.uint32) != got.view(np.uint32)) | (dec != T["decision"]) | (nl != T["left_count"]) | (nr != T["right_count"]))
    if len(bad[0]):
        _fail("a cost-table entry is not what its children's entries give", [
            "node %d entry %d: (%r, %d, %d, %d) for (%r, %d, %d, %d)" % (x, i, got[x, i], T["decision"][x, i], T["left_count"][x, i], T["right_count"][x, i], cost[x, i], dec[x, i], nl[x, i], nr[x, i])
            for x, i in zip(*bad)])
    C = cost_table64(T, levels)
    want = C[:n - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(want > 0, np.abs(got.astype(np.float64) - want) / want, np.where(got == 0, 0.0, np.inf))
    bound = dp_bound(len(levels))
    bad = np.nonzero(dev > bound)
    if len(bad[0]):
        _fail("a cost is further than %.3g from the float64 programme" % bound, ["node %d entry %d: %r for %r" % (x, i, got[x, i], want[x, i]) for x, i in zip(*bad)])
    return C, float(dev.max())


# ---- (f) collapse ---------------------------------------------------------------------------------------------------------
def _entry(T, x, i):
    """(decision, left_count, right_count) of eval_of(x, i)"""
    if x >= T["n"] - 1:
        return DEC_LEAF, 0, 0
    return int(T["decision"][x, i]), int(T["left_count"][x, i]), int(T["right_count"][x, i])


def gather_children(T, x, follow_distribute=True):
    """the children of the wide node over binary node x, in the kernel's order: a stack, left pushed before right.
    follow_distribute=False is a planted defect: a 'distribute' entry taken for a child."""
    child, todo = [], [(x, 0)]
    while todo:
        y, i = todo.pop()
        _, nl, nr = _entry(T, y, i)
        for side, si in ((int(T["left"][y]), nl), (int(T["right"][y]), nr)):
            if follow_distribute and _entry(T, side, si)[0] == DEC_DISTRIBUTE and len(todo) < 8:
                todo.append((side, si))
            elif len(child) < 8:
                child.append(side)
    return child


def is_inner(T, c):
    if c >= T["n"] - 1:
        return False
    return bool(T["count"][c] > LEAF_MAX or T["decision"][c, 0] == DEC_INTERNAL)


def assign_slots(T, x, child):
    """child_at[slot] = position in `child` or -1: the greedy rule, repeatedly the free (child, slot) pair with the smallest
    dot(child centre - node centre, slot direction) in binary32 (products with +-1 are exact), the first such pair in (child, slot) order"""
    box = np.asarray(T["box"], F)
    nc = centres(box[x, 0], box[x, 1])
    d = (centres(box[child, 0], box[child, 1]) - nc).astype(F)
    sign = np.array([[-1.0 if s & 4 else 1.0, -1.0 if s & 2 else 1.0, -1.0 if s & 1 else 1.0] for s in range(8)], F)
    cost = (((d[:, None, 0] * sign[None, :, 0]).astype(F) + (d[:, None, 1] * sign[None, :, 1]).astype(F)).astype(F) + (d[:, None, 2] * sign[None, :, 2]).astype(F)).astype(F)
    cost = cost.astype(np.float64)  # (exact; +inf marks what is taken)
    child_at = [-1] * 8
    for _ in range(len(child)):
        k, s = np.unravel_index(int(np.argmin(cost)), cost.shape)
        child_at[s] = int(k)
        cost[k, :] = np.inf
        cost[:, s] = np.inf
    return child_at


def frame_of(lo, hi):
    """(e bytes [3], inverse scale f32 [3]) of the node box: e = ceil(log2(extent / 255)), raised by one where 255 * 2^e < extent"""
    e, inv = np.zeros(3, np.uint8), np.zeros(3, F)
    for a in range(3):
        ext = F(F(hi[a]) - F(lo[a]))
        with np.errstate(divide="ignore"):
            ex = float(np.ceil(F(np.log2(np.float64(F(ext * F(F(1.0) / F(255.0))))))))
        if abs(ex) < 126.0 and F(F(255.0) * F(np.ldexp(F(1.0), int(ex)))) < ext:
            ex += 1.0
        e[a] = 0 if not ex > -127.0 else (255 if ex >= 128.0 else int(ex) + 127)
        pw = 0.0 if ex < -200.0 else (np.inf if ex > 200.0 else float(np.ldexp(1.0, int(ex))))
        with np.errstate(divide="ignore"):
            inv[a] = F(1.0) / F(pw)
    return e, inv


def _quantize(v):
    v = np.asarray(v, F)
    return np.where(v != v, 0, np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0)).astype(np.uint8)


def replay_node(T, x, follow_distribute=True):
    """What collapse_level_kernel writes for the wide node over binary node x, but for childBaseIdx / triangleBaseIdx:
    dict of p [3], e [3], imask, meta [8], qlo / qhi [8, 3], inner [(slot, binary node)] in slot order, leaf {slot: [primitives]}"""
    n = T["n"]
    box = np.asarray(T["box"], F)
    child = gather_children(T, x, follow_distribute)
    child_at = assign_slots(T, x, child)
    e, inv = frame_of(box[x, 0], box[x, 1])
    out = {"p": box[x, 0].copy(), "e": e, "imask": 0, "meta": np.zeros(8, np.uint8), "qlo": np.zeros((8, 3), np.uint8), "qhi": np.zeros((8, 3), np.uint8),
           "inner": [], "leaf": {}, "leaf_node": {}}
    seen = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(8):
            if child_at[s] < 0:
                continue
            c = child[child_at[s]]
            out["qlo"][s] = _quantize(np.floor(((box[c, 0] - box[x, 0]).astype(F) * inv).astype(F)))
            out["qhi"][s] = _quantize(np.ceil(((box[c, 1] - box[x, 0]).astype(F) * inv).astype(F)))
            if is_inner(T, c):
                out["meta"][s] = 0x20 | (24 + s)
                out["imask"] |= 1 << s
                out["inner"].append((s, c))
            else:
                leaves, todo = [], [c]
                while todo and len(leaves) < 3:
                    y = todo.pop()
                    if y >= n - 1:
                        leaves.append(y - (n - 1))
                    else:
                        todo += [int(T["right"][y]), int(T["left"][y])]
                tris = 1 if c >= n - 1 else int(T["count"][c])
                out["meta"][s] = ((1 << tris) - 1) << 5 | seen
                out["leaf"][s] = [int(T["leaf_order"][k]) for k in leaves[:tris]]
                out["leaf_node"][s] = c
                seen += tris
    return out


_Q = ("qlox", "qloy", "qloz", "qhix", "qhiy", "qhiz")


def check_collapse(T, nodes, prim_idx, C=None, height=None):
    """Walk the replay and the wide nodes together from the root.  With C (check_cost_table's float64 table): the float64 cost of the wide
    tree — area per wide node, area * count * primCost per leaf slot, areas of the binary tree's boxes — against C(root, 0).
    -> (wide nodes walked, total / C(root, 0) - 1)"""
    n = T["n"]
    box64 = np.asarray(T["box"], np.float64)
    area = half_area64(box64[:, 0], box64[:, 1])
    pc = float(F(T["prim_cost"]))
    prim_idx = np.asarray(prim_idx, np.int64)
    todo, walked, total, fails = [(0, 0)], 0, 0.0, []
    while todo and len(fails) < 4:
        x, w = todo.pop()
        if w >= len(nodes) or walked > len(nodes):
            fails.append("binary node %d: its wide node %d is past the %d nodes" % (x, w, len(nodes)))
            break
        walked += 1
        total += area[x]
        want, got = replay_node(T, x), nodes[w]
        where = "wide node %d (binary node %d)" % (w, x)
        if int(got["imask"]) != want["imask"] or not np.array_equal(np.asarray(got["meta"], np.uint8), want["meta"]):
            fails.append("%s: imask %02x meta %s, the replay %02x %s" % (where, int(got["imask"]), [hex(int(v)) for v in got["meta"]], want["imask"], [hex(int(v)) for v in want["meta"]]))
            continue
        if not np.array_equal(np.asarray(got["p"], F).view(np.uint32), want["p"].view(np.uint32)) or not np.array_equal(np.asarray(got["e"], np.uint8), want["e"]):
            fails.append("%s: frame p %s e %s, the replay %s %s" % (where, got["p"], got["e"], want["p"], want["e"]))
        q = np.stack([np.asarray(got[f], np.uint8) for f in _Q], axis=1)
        if not np.array_equal(q[:, :3], want["qlo"]) or not np.array_equal(q[:, 3:], want["qhi"]):
            fails.append("%s: quantised boxes %s, the replay %s" % (where, q.tolist(), np.concatenate([want["qlo"], want["qhi"]], axis=1).tolist()))
        for s, prims in want["leaf"].items():
            at = int(got["triangleBaseIdx"]) + (int(want["meta"][s]) & 31)
            have = prim_idx[at:at + len(prims)].tolist()
            if have != prims:
                fails.append("%s slot %d: primitives %s, the replay %s" % (where, s, have, prims))
            total += area[want["leaf_node"][s]] * len(prims) * pc
        for rank, (s, c) in enumerate(want["inner"]):
            todo.append((c, int(got["childBaseIdx"]) + rank))
    if not fails and walked != len(nodes):
        fails.append("%d wide nodes walked, %d read back" % (walked, len(nodes)))
    if fails:
        _fail("the collapse", fails)
    excess = 0.0
    if C is not None:
        excess = total / C[0, 0] - 1.0 if C[0, 0] > 0 else 0.0
        bound = dp_bound(height)
        if not -bound <= excess <= bound:
            _fail("the wide tree costs %.9g, the programme's optimum is %.9g (%.3g apart, bound %.3g): the walk does not follow the table" % (total, C[0, 0], excess, bound))
    return walked, excess


def check_all(T, plo, phi, nodes, prim_idx):
    """(a), the builder's own check, (e), (f) -> dict of the figures"""
    builder = T["builder"]
    levels = levels_of(T)
    loose, sah_excess = (check_sah(T, plo, phi, levels) if builder < 0 else (None, 0.0))
    levels, height = check_structure(T, plo, phi, loose)
    if builder == 0:
        check_radix(T, plo, phi, levels)
    elif builder > 0:
        check_clustering(T, plo, phi, builder)
    C, dp_dev = check_cost_table(T, levels)
    walked, excess = check_collapse(T, nodes, prim_idx, C, height)
    return {"height": height, "sah_excess": sah_excess, "dp_deviation": dp_dev, "wide_nodes": walked, "collapse_excess": excess}


# ---- inputs both test modules use -------------------------------------------------------------------------------------------
def boxes_of(tris):
    """(lo, hi) [n, 3] binary32: min / max of the corners, exact"""
    lo = np.minimum(np.minimum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(F)
    hi = np.maximum(np.maximum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(F)
    return lo, hi


def ribbon(n):
    """n triangles in a row along x, alternately up and down"""
    from nexus_amd import pod

    k = np.arange(n, dtype=np.float64)
    p = np.zeros((n, 3, 3))
    p[:, 0] = np.stack([0.1 * k, 0.02 * (k % 3), 0.0 * k], 1)
    p[:, 1] = np.stack([0.1 * k + 0.1, 0.0 * k, 0.03 * (k % 5)], 1)
    p[:, 2] = np.stack([0.1 * k + 0.05, 0.1 + 0.01 * (k % 2), 0.0 * k], 1)
    return pod.make_triangles(p.astype(F))


def copies_and_distinct(copies, distinct, seed=6):
    """`copies` times one triangle, then `distinct` different ones: equal Morton codes, nodes that nothing separates"""
    from nexus_amd import scenegen

    return np.concatenate([np.repeat(scenegen.random_soup(1, seed=seed), copies), scenegen.random_soup(distinct, seed=seed + 1)])


def planar_grid(m):
    """2 m^2 triangles of a flat grid in the plane z = 0: a dead axis for the binning"""
    from nexus_amd import scenegen

    t = scenegen.height_field(m, seed=7, amp=0.0).copy()
    for f in ("pos0", "pos1", "pos2"):
        t[f] = t[f][:, [0, 2, 1]]
    return t
