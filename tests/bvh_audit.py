"""Exact audit of the 80-byte wide-BVH nodes: structure, quantisation frame, containment and tightness of EVERY slot box.

TEST INFRASTRUCTURE ONLY.  The module reads node bytes and primitive boxes and nothing else: it imports no builder (neither the
product's nor the oracle's) and restates none, so a mistake shared by the builders cannot hide in it.

Arithmetic.  Every finite binary32 number is an integer multiple of 2^-149, and so is every grid step 2^(e-127) with an exponent
byte e >= 1.  All quantities below are therefore Python integers in units of 2^-149 (`_ints`: a binary32 scaled by the power of
two 2^149 in float64 is exact and in range, and int() of a float64 is exact).  No comparison in the exact audit rounds.
  decoded lo = p + qlo * 2^(e-127),  decoded hi = p + qhi * 2^(e-127)          (exact)
  true box of a node = min / max over the primitive boxes of its subtree, bottom-up (a union of binary32 numbers is exact)
  L, H of a slot = true box of the child node (inner slot) or of the slot's 1..3 primitives (leaf slot)

What a builder may do, from its text (`q = floor((x - p) * invScale)`, `ceil` for the upper face, invScale = 2^-(e-127)):
  * `x - p` is ONE binary32 subtraction: fl(x - p) = (x - p)(1 + d), |d| <= 2^-24.
  * the multiplication by a power of two is exact (no overflow or underflow on these meshes), floor / ceil are exact, and the
    clamp to [0, 255] does nothing once 255 * 2^(e-127) >= extent (see the exponent rule).
  hence   decoded lo = p + floor(fl(L - p) / step) * step  <=  p + fl(L - p)  <=  L + 2^-24 (L - p)
          decoded lo                                       >   p + fl(L - p) - step  >=  L - 2^-24 (L - p) - step
  and, mirrored, decoded hi >= H - 2^-24 (H - p) and decoded hi < H + 2^-24 (H - p) + step.
  delta = 2^-24 * (coordinate - p) is the whole allowance; it is derived, not measured, and is zero on a frame's own origin.
  Comparisons are made after multiplying through by 2^24, so they stay in integers.

Frame.  p must equal the true minimum of the node on every axis (as a number: a zero of either sign is the same origin).
With k = e - 127 the exponent must satisfy 255 * 2^k >= fl32(extent) exactly, where extent = true max - true min and fl32 is the
one binary32 subtraction the builders take everything from (`_fl32`: round to nearest even, computed on the integers).  The exact
extent may exceed 255 * 2^k by that rounding alone, less than 2^-24 of itself; the slot boxes then are short of the far face by
the same amount, which is the delta above, and `rounded_frames` counts such frames.  (An instance record's boundsMax is itself
fl32(p + 255 * 2^e) of its BLAS root, so a TLAS over a single instance meets this on about every second axis.)  Where max - min is
exact in binary32 — every frame of the boundary family — the rule is 255 * 2^k >= extent with no allowance at all.
k must also be the smallest such exponent: 255 * 2^(k-1) < extent — except inside the rounding window of the builders' expression
  e = ceil(fl32(log2(fl(fl(hi - lo) * fl(1 / 255))))),
where three binary32 roundings (subtraction, the constant 1/255 which rounds up, the product) scale the argument by at most
(1 + 2^-24)^3 and the binary32 logarithm is off by at most one ulp u of its value k - 1 (glibc: 0.75 ulp; a correctly rounded one:
0.5).  2^u <= 1 + u for 0 <= u <= 1, so an exponent one too large is accepted only if
  extent * (1 + 2^-24)^3 * (1 + ulp32(k - 1)) >= 255 * 2^(k-1)               (evaluated in fractions)
with ulp32(0) taken as 0 (log2 of a number just above 1 is positive whatever its rounding).  An axis of zero extent has exponent
byte 0 — the documented degenerate axis — and every slot on it decodes to p.

The second entry point, `audit_tlas_geometry`, is for a TLAS built on the device from tightened instance boxes that cannot be read
back: structure as above; containment of leaf AND inner slots against float64 world-space geometry with the slack the suite has
always used for that comparison (1e-5 * max(1, |decoded hi|)); looseness of an inner slot against the exact union U of its
subtree's decoded leaf slots: decoded lo > U.lo - step - 2 delta, decoded hi < U.hi + step + 2 delta (one subtraction rounding
where the leaf slot was quantised, one where this slot was; a leaf's frame origin is not below its ancestors', so
delta = 2^-24 (U - p) with this node's p bounds both).
"""
from fractions import Fraction

import numpy as np

_UNIT = 149          # integers count multiples of 2^-149
_SH = 24             # delta = 2^-24 * (coordinate - p)
_Q_FIELDS = ("qlox", "qloy", "qloz", "qhix", "qhiy", "qhiz")


class AuditError(AssertionError):
    def __init__(self, failures, report):
        self.failures, self.report = failures, report
        AssertionError.__init__(self, "%d audit failure(s); first: %s" % (len(failures), "; ".join(failures[:4])))


class Report:
    """Worst containment shortfall and worst looseness over all slots and axes, each in grid steps of the node and in binary32 ulp
    of the coordinate it was measured at; `failures` lists what broke a rule."""

    def __init__(self):
        self.nodes = self.slots = 0
        self.short_steps = self.short_ulp = self.loose_steps = self.loose_ulp = 0.0
        self.short_at = self.loose_at = None
        self.wide_exponents = 0  # frames one exponent above the minimum, inside the logarithm's rounding window
        self.rounded_frames = 0  # frames whose exact extent exceeds 255 steps by the rounding of max - min alone
        self.rounded_worst_steps = 0.0
        self.failures = []

    def line(self, what=""):
        text = "%s: %d nodes, %d slots; worst shortfall %.3g step = %.3g ulp%s; worst looseness %.4g step = %.4g ulp%s" % (
            what, self.nodes, self.slots, self.short_steps, self.short_ulp, " at node,slot,axis %s" % (self.short_at,) if self.short_at else "",
            self.loose_steps, self.loose_ulp, " at %s" % (self.loose_at,) if self.loose_at else "")
        if self.wide_exponents:
            text += "; %d frame exponent(s) one above the minimum" % self.wide_exponents
        if self.rounded_frames:
            text += "; %d frame(s) whose exact extent is up to %.3g step above 255 steps by the rounding of max - min" % (self.rounded_frames, self.rounded_worst_steps)
        return text


def _ints(a):
    """binary32 array -> object array of Python integers, value / 2^-149 (exact)"""
    a = np.asarray(a, dtype=np.float32)
    if not np.all(np.isfinite(a)):
        raise AuditError(["a coordinate is not a finite number"], Report())
    scaled = np.ldexp(a.astype(np.float64), _UNIT)  # power-of-two scaling of a binary32 in binary64: exact, |result| < 2^277
    out = np.empty(a.size, dtype=object)
    out[:] = [int(v) for v in scaled.ravel()]
    return out.reshape(a.shape)


def _fl32(v):
    """a non-negative integer (units of 2^-149) rounded to binary32, nearest even: what one binary32 subtraction returns"""
    if v < (1 << 24):
        return v
    sh = v.bit_length() - 24
    q, r = divmod(v, 1 << sh)
    half = 1 << (sh - 1)
    if r > half or (r == half and q & 1):
        q += 1
    return q << sh


def _ulp32_units(x_units):
    """spacing of binary32 at the value x (units of 2^-149), as an integer of the same units"""
    m = abs(int(x_units))
    return 1 if m < (1 << 24) else 1 << (m.bit_length() - 24)


def triangle_boxes(tris):
    lo = np.minimum(np.minimum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(np.float32)
    hi = np.maximum(np.maximum(tris["pos0"], tris["pos1"]), tris["pos2"]).astype(np.float32)
    return lo, hi


def instance_boxes(instances):
    return np.asarray(instances["boundsMin"], np.float32), np.asarray(instances["boundsMax"], np.float32)


def _structure(nodes, idx, prim_count, tlas, fails):
    """Walk from the root: every node once, every primitive once, meta encodings, 1..3 primitives per leaf slot, at most 24 per
    node, inner children on consecutive node numbers in slot order (childBaseIdx + rank), behind their parent in a TLAS.
    -> (nodes in breadth-first order, kind[n][s]: 0 empty / 1 leaf / 2 inner, ref[n][s]: child node or (first, count))"""
    n = len(nodes)
    idx = np.asarray(idx)
    if len(idx) != prim_count or sorted(idx.tolist()) != list(range(prim_count)):
        fails.append("the index list is not a permutation of the %d primitives" % prim_count)
        return None
    if n == 0:
        fails.append("no nodes")
        return None
    imask, meta_all = nodes["imask"], nodes["meta"]
    cbase, tbase = nodes["childBaseIdx"], nodes["triangleBaseIdx"]
    kind = [[0] * 8 for _ in range(n)]
    ref = [[None] * 8 for _ in range(n)]
    seen_node = [False] * n
    seen_prim = [False] * prim_count
    seen_node[0] = True
    order = [0]
    at = 0
    while at < len(order):
        ni = order[at]
        at += 1
        im, total, rank = int(imask[ni]), 0, 0
        for s in range(8):
            meta = int(meta_all[ni][s])
            if im >> s & 1:
                if meta != (0x20 | (24 + s)):
                    fails.append("node %d slot %d: inner slot with meta 0x%02x" % (ni, s, meta))
                    return None
                c = int(cbase[ni]) + rank
                rank += 1
                if c >= n or seen_node[c]:
                    fails.append("node %d slot %d: child %d out of range or reached twice" % (ni, s, c))
                    return None
                if tlas and c <= ni:
                    fails.append("node %d slot %d: child %d is not behind its parent" % (ni, s, c))
                    return None
                seen_node[c] = True
                order.append(c)
                kind[ni][s], ref[ni][s] = 2, c
            elif meta:
                cnt = bin(meta >> 5).count("1")
                if (meta >> 5) != (1 << cnt) - 1 or not 1 <= cnt <= 3:
                    fails.append("node %d slot %d: leaf meta 0x%02x is not a unary count of 1..3" % (ni, s, meta))
                    return None
                first = int(tbase[ni]) + (meta & 0x1F)
                if first + cnt > prim_count:
                    fails.append("node %d slot %d: primitives %d..%d past the list" % (ni, s, first, first + cnt - 1))
                    return None
                for k in range(first, first + cnt):
                    if seen_prim[k]:
                        fails.append("node %d slot %d: list entry %d referenced twice" % (ni, s, k))
                        return None
                    seen_prim[k] = True
                total += cnt
                kind[ni][s], ref[ni][s] = 1, (first, cnt)
        if total > 24:
            fails.append("node %d holds %d primitives" % (ni, total))
        if total == 0 and rank == 0:
            fails.append("node %d is empty" % ni)
            return None
    if not all(seen_node):
        fails.append("%d node(s) not reached from the root" % seen_node.count(False))
        return None
    if not all(seen_prim):
        fails.append("%d list entries referenced by no slot" % seen_prim.count(False))
        return None
    return order, kind, ref


def _decoded(nodes):
    """(P ints (N,3), step ints (N,3), decoded lo / hi ints (N,8,3))"""
    N = len(nodes)
    P = _ints(nodes["p"])
    e = nodes["e"].astype(np.int64)
    step = np.empty((N, 3), dtype=object)
    step.ravel()[:] = [0 if b == 0 else 1 << (int(b) + 22) for b in e.ravel()]  # 2^(e-127) / 2^-149
    q = [np.asarray(nodes[f]).astype(np.int64).astype(object) for f in _Q_FIELDS]
    qlo = np.stack(q[:3], axis=-1)
    qhi = np.stack(q[3:], axis=-1)
    dlo = P[:, None, :] + qlo * step[:, None, :]
    dhi = P[:, None, :] + qhi * step[:, None, :]
    return P, step, dlo, dhi


def _window_allows(ext_units, step_units, k):
    """is an exponent k one above the minimum inside the rounding window of the builders' logarithm (module docstring)?"""
    km1 = abs(k - 1)
    u = Fraction(0) if km1 == 0 else Fraction(float(np.spacing(np.float32(km1))))
    return Fraction(ext_units) * (1 + Fraction(1, 1 << 24)) ** 3 * (1 + u) >= Fraction(255 * step_units, 2)


def audit(nodes, idx, prim_lo, prim_hi, tlas=False, check=True, built=True):
    """Exact audit of a BLAS (primitive boxes = triangle boxes) or of a host-built / host-refitted TLAS (primitive boxes = the
    instance records' boundsMin / boundsMax).  Returns a Report; raises AuditError when a rule is broken and `check` is set.
    built=False is for a tree encoded by hand (tests/bvh_craft.py), whose frames are whatever its author chose: structure and
    exact containment of every slot only, no rule about the frame's origin, its exponent or the boxes' tightness."""
    rep = Report()
    fails = rep.failures
    nodes = np.asarray(nodes)
    walk = _structure(nodes, idx, len(prim_lo), tlas, fails)
    if walk is None:
        if check:
            raise AuditError(fails, rep)
        return rep
    order, kind, ref = walk
    N = len(nodes)
    idx = [int(i) for i in np.asarray(idx)]
    plo, phi = _ints(prim_lo).tolist(), _ints(prim_hi).tolist()
    # true boxes, children before parents
    L = np.zeros((N, 8, 3), dtype=object)
    H = np.zeros((N, 8, 3), dtype=object)
    used = np.zeros((N, 8), dtype=bool)
    box_lo, box_hi = [None] * N, [None] * N
    for ni in reversed(order):
        nlo = nhi = None
        for s in range(8):
            kd = kind[ni][s]
            if kd == 0:
                continue
            if kd == 2:
                lo, hi = box_lo[ref[ni][s]], box_hi[ref[ni][s]]
            else:
                first, cnt = ref[ni][s]
                ps = [idx[k] for k in range(first, first + cnt)]
                lo = [min(plo[t][a] for t in ps) for a in range(3)]
                hi = [max(phi[t][a] for t in ps) for a in range(3)]
            used[ni, s] = True
            L[ni, s, :], H[ni, s, :] = lo, hi
            nlo = lo if nlo is None else [min(x, y) for x, y in zip(nlo, lo)]
            nhi = hi if nhi is None else [max(x, y) for x, y in zip(nhi, hi)]
        box_lo[ni], box_hi[ni] = nlo, nhi
    BL = np.array(box_lo, dtype=object).reshape(N, 3)
    BH = np.array(box_hi, dtype=object).reshape(N, 3)
    P, step, dlo, dhi = _decoded(nodes)
    rep.nodes, rep.slots = N, int(used.sum())

    # frame origin
    for ni, a in zip(*np.nonzero(P != BL)) if built else ():
        fails.append("node %d axis %d: frame origin is %+d units of 2^-149 from the subtree's minimum" % (ni, a, P[ni, a] - BL[ni, a]))
    # frame exponent
    ext = BH - BL
    e = nodes["e"]
    for ni, a in zip(*np.nonzero((ext == 0) != (step == 0))) if built else ():
        fails.append("node %d axis %d: exponent byte %d with extent %s zero" % (ni, a, e[ni, a], "equal to" if ext[ni, a] == 0 else "above"))
    live = (ext != 0) & (step != 0) & built
    for ni, a in zip(*np.nonzero(live & (255 * step < ext))):
        over = float(Fraction(ext[ni, a] - 255 * step[ni, a], step[ni, a]))
        if 255 * step[ni, a] < _fl32(ext[ni, a]):
            fails.append("node %d axis %d: 255 * 2^%d is %.3g step short of the extent" % (ni, a, int(e[ni, a]) - 127, over))
        else:
            rep.rounded_frames += 1
            rep.rounded_worst_steps = max(rep.rounded_worst_steps, over)
    for ni, a in zip(*np.nonzero(live & (255 * step >= 2 * ext))):
        k = int(e[ni, a]) - 127
        if 255 * step[ni, a] < 4 * ext[ni, a] and _window_allows(ext[ni, a], step[ni, a], k):
            rep.wide_exponents += 1
        else:
            fails.append("node %d axis %d: exponent 2^%d although 255 * 2^%d covers the extent" % (ni, a, k, k - 1))

    # containment and tightness of every used slot, inner and leaf alike
    U = np.repeat(used[:, :, None], 3, axis=2)
    Pb = np.broadcast_to(P[:, None, :], (N, 8, 3))
    Sb = np.broadcast_to(step[:, None, :], (N, 8, 3))
    flat = Sb == 0
    short_lo, short_hi = dlo - L, H - dhi        # > 0: the box ends inside what it bounds
    loose_lo, loose_hi = L - dlo, dhi - H        # > 0: the box is wider than what it bounds
    scale = 1 << _SH
    bad_in = U & ~flat & ((short_lo * scale > (L - Pb)) | (short_hi * scale > (H - Pb)))
    bad_out = U & ~flat & (((loose_lo - Sb) * scale >= (L - Pb)) | ((loose_hi - Sb) * scale >= (H - Pb)))
    bad_flat = U & flat & ((dlo != L) | (dhi != H))
    if not built:
        bad_out = np.zeros_like(bad_out)
    for what, bad in (("ends inside what it bounds", bad_in), ("is a step or more too wide", bad_out), ("on a degenerate axis is not the plane", bad_flat)):
        for ni, s, a in list(zip(*np.nonzero(bad)))[:8]:
            fails.append("node %d slot %d (%s) axis %d %s: decoded [%d, %d], true [%d, %d], step %d (units of 2^-149)" % (
                ni, s, "inner" if kind[ni][s] == 2 else "leaf", a, what, dlo[ni, s, a], dhi[ni, s, a], L[ni, s, a], H[ni, s, a], Sb[ni, s, a]))
        if bad.sum() > 8:
            fails.append("... and %d more slots whose box %s" % (int(bad.sum()) - 8, what))

    # the figures
    live3 = U & ~flat
    if live3.any():
        sf = np.where(live3, Sb, 1).astype(np.float64)
        for name, lo_side, hi_side in (("short", short_lo, short_hi), ("loose", loose_lo, loose_hi)):
            r = np.maximum(np.where(live3, lo_side, 0).astype(np.float64), np.where(live3, hi_side, 0).astype(np.float64)) / sf
            w = np.unravel_index(int(np.argmax(r)), r.shape)
            if r[w] > 0:
                from_lo = lo_side[w] >= hi_side[w]
                amount = lo_side[w] if from_lo else hi_side[w]
                coord = L[w] if from_lo else H[w]
                setattr(rep, name + "_steps", float(Fraction(amount, Sb[w])))
                setattr(rep, name + "_ulp", float(Fraction(amount, _ulp32_units(coord))))
                setattr(rep, name + "_at", tuple(int(x) for x in w))
    if fails and check:
        raise AuditError(fails, rep)
    return rep


def audit_tlas_geometry(nodes, idx, geo_lo, geo_hi, check=True):
    """A TLAS whose builder worked from boxes that cannot be read back (the device build's tightened instance boxes): structure;
    every slot, inner and leaf, contains the float64 world-space geometry (geo_lo, geo_hi per instance) of its subtree within
    1e-5 * max(1, |decoded hi|); an inner slot is no wider than the union of its subtree's decoded leaf slots plus one step (and
    the two subtraction roundings of the module docstring)."""
    rep = Report()
    fails = rep.failures
    nodes = np.asarray(nodes)
    geo_lo, geo_hi = np.asarray(geo_lo, np.float64), np.asarray(geo_hi, np.float64)
    walk = _structure(nodes, idx, len(geo_lo), True, fails)
    if walk is None:
        if check:
            raise AuditError(fails, rep)
        return rep
    order, kind, ref = walk
    N = len(nodes)
    idx = np.asarray(idx).astype(np.int64)
    P, step, dlo, dhi = _decoded(nodes)
    flo = np.ldexp(dlo.astype(np.float64), -_UNIT)  # the decoded boxes as binary64 (one rounding each: this leg compares with slack)
    fhi = np.ldexp(dhi.astype(np.float64), -_UNIT)
    rep.nodes = N
    g_lo, g_hi = [None] * N, [None] * N      # geometry under a node
    u_lo, u_hi = [None] * N, [None] * N      # exact union of the decoded leaf slots under a node
    scale = 1 << _SH
    for ni in reversed(order):
        for s in range(8):
            kd = kind[ni][s]
            if kd == 0:
                continue
            rep.slots += 1
            if kd == 2:
                c = ref[ni][s]
                wl, wh, ul, uh = g_lo[c], g_hi[c], u_lo[c], u_hi[c]
            else:
                first, cnt = ref[ni][s]
                ps = idx[first:first + cnt]
                wl, wh = geo_lo[ps].min(0), geo_hi[ps].max(0)
                ul, uh = list(dlo[ni, s]), list(dhi[ni, s])
            eps = 1e-5 * np.maximum(1.0, np.abs(fhi[ni, s]))
            if not (np.all(flo[ni, s] <= wl + eps) and np.all(fhi[ni, s] >= wh - eps)):
                fails.append("node %d slot %d (%s): decoded [%s, %s] does not contain the geometry [%s, %s]" % (ni, s, "inner" if kd == 2 else "leaf", flo[ni, s], fhi[ni, s], wl, wh))
            short = float(max(np.max((flo[ni, s] - wl)), np.max(wh - fhi[ni, s]), 0.0))
            st = float(min(np.ldexp(float(x), -_UNIT) for x in step[ni] if x)) if short > 0.0 and any(step[ni]) else 0.0
            if st and short / st > rep.short_steps:
                rep.short_steps, rep.short_at = short / st, (ni, s)
                rep.short_ulp = short / float(np.spacing(np.float32(np.max(np.abs(fhi[ni, s])))))
            if kd == 2:
                for a in range(3):
                    sa, pa = step[ni, a], P[ni, a]
                    too_lo = (ul[a] - dlo[ni, s, a] - sa) * scale >= 2 * abs(ul[a] - pa) and not (sa == 0 and ul[a] == dlo[ni, s, a])
                    too_hi = (dhi[ni, s, a] - uh[a] - sa) * scale >= 2 * abs(uh[a] - pa) and not (sa == 0 and uh[a] == dhi[ni, s, a])
                    if too_lo or too_hi:
                        fails.append("node %d slot %d axis %d: inner box [%d, %d] is a step or more wider than its leaves' union [%d, %d], step %d" % (ni, s, a, dlo[ni, s, a], dhi[ni, s, a], ul[a], uh[a], sa))
                    if sa:
                        over = max(ul[a] - dlo[ni, s, a], dhi[ni, s, a] - uh[a])
                        if over > 0 and float(Fraction(over, sa)) > rep.loose_steps:
                            rep.loose_steps, rep.loose_at = float(Fraction(over, sa)), (ni, s, a)
                            rep.loose_ulp = float(Fraction(over, _ulp32_units(uh[a])))
            if g_lo[ni] is None:
                g_lo[ni], g_hi[ni], u_lo[ni], u_hi[ni] = wl, wh, list(ul), list(uh)
            else:
                g_lo[ni], g_hi[ni] = np.minimum(g_lo[ni], wl), np.maximum(g_hi[ni], wh)
                u_lo[ni] = [min(x, y) for x, y in zip(u_lo[ni], ul)]
                u_hi[ni] = [max(x, y) for x, y in zip(u_hi[ni], uh)]
    if fails and check:
        raise AuditError(fails, rep)
    return rep
