"""The camera in float64, from its parameters — the reference of tests/test_camera_reference.py (CPU) and tests/test_gpu_camera.py.

Written from the camera's definition, not from the code: no product module, no oracle, no nx_camera struct is read here.

THE MODEL.  A camera is position, forward (unit), horizontal field of view, image size W x H, focus distance and defocus angle; the
parameters are binary32 numbers (what the interface takes) and everything below is binary64.
  basis      right = normalize(forward x world_up), up = right x forward, world_up = (0, 1, 0).
             quirk=True: right = forward x world_up NOT normalised — what Camera's constructor and LookAt do (and the reference's
             constructor): for a forward pitched by theta, |right| = |up| = cos theta.
  rectangle  in the focal plane: centre position + focus forward, half width a = focus tan(hfov / 2) along right, half height
             a H / W along up.  Pixel (i, j) covers [i / W, (i + 1) / W) x [j / H, (j + 1) / H) of it measured from the lower-left corner:
             image row 0 is the bottom row (include/nexus_hip.h, nxhip_debug_read_primary_rays).
  numbers    Jenkins' one-at-a-time hash h; state s0 = h(((i + j W) xor h(frame)) or 1 when that is 0); xorshift 13 / 17 / 5 per draw;
             value (s >> 9) 2^-23.  uint32 arithmetic, exact: no tolerance applies to a random number.
  draws      jitter x, jitter y, then pairs (a, b) for the lens: p = 2 (a - 1/2, b - 1/2), the first pair with |p| < 1.  p and |p|^2 are
             exact in binary64; a pair with | |p|^2 - 1 | <= 4 x 2^-23 marks the path `unclear` (binary32 forms |p| with three roundings
             of at most 2^-24 each and a square root: its decision may differ there, and every later number of the path with it).
  ray        origin = position + R (p.x right + p.y up), R = focus tan(defocus / 2);  direction = normalize(F - origin),
             F = corner + (i + jx) / W (2a right) + (j + jy) / H (2a H / W up) the jittered point of the rectangle.

THE BOUNDS (u = 2^-24, the unit roundoff of binary32; vector errors as Euclidean norms: rounding a vector r costs at most u |r|).
Camera::ToDevice, in binary32:
  t = tan(float(deg / 2 * pi / 180)): the argument carries 1 u, which tan turns into K u with K = 2x / sin 2x (x the half angle: 1.00
      at 2.5 deg, 2.42 at 60 deg), plus 2 u for a tanf good to one unit in the last place: e_t = K + 2.
  halfWidth = focus t: e_t + 1.  halfHeight = halfWidth / (W / float(H)): e_t + 3.
  right = (-f.z, 0, f.x): exact in the code, which does not normalise it — but forward is a unit vector ROUNDED to binary32, 1 within u
      long, and the model normalises: 1 u on right, and on everything made from it.
      up = right x forward = (-r.z f.y, r.z f.x - r.x f.z, r.x f.y): the middle component is f.x^2 + f.z^2, a sum of two positive
      products — at most 3 u on every component, 4 u with right's.
  viewportX = (2 halfWidth) right: (e_t + 3) u |vpX|.   viewportY = (2 halfHeight) up: (e_t + 8) u |vpY|.
  lowerLeftCorner = ((position - vpX / 2) - vpY / 2) + forward focus: halves are exact; the four roundings act on vectors no longer
      than 1.5 M, 2 M, focus <= 3 M and M, with M = max(|llc|, |position|, |vpX|, |vpY|, |offset|): 7.5 u M.
generate_kernel, in binary32, for the point ((llc + vpX x) + vpY y) - position - offset:
  inherited  vpX enters as (x - 1/2) vpX, vpY as (y - 1/2) vpY (the corner holds -1/2 of each): (e_t + 3) / 2 + (e_t + 8) / 2, and the
             corner's own 7.5: (e_t + 13) u M.
  x, y       (i + r) / W: two roundings each, 2 u |vpX| + 2 u |vpY| <= 4 u M.
  products   vpX x, vpY y: 2 u M.   sums  llc + vpX x: a vector within 2 M; + vpY y: within 3 M: 5 u M.
  - position the result is v0 = F - position: u |v0| <= u (|v| + |offset|).   - offset: u |v|.
  offset     R carries e_R = K' + 3 (K' <= 1.006 up to 10 degrees of defocus); rdx, rdy one more; right rdx: e_R + 3 on |right rdx|;
             up rdy: e_R + 6 on |up rdy| (up's 4 u); the sum: u |offset|.  With |right rdx| + |up rdy| <= sqrt 2 |offset| (orthogonal
             axes of equal length): ((e_R + 6) sqrt 2 + 1) u |offset| <= 15.2 u |offset| <= 15.2 u M.
  Together   |error of v| <= u ((K + 26 + 15.2) M + 2 |v| + |offset|) <= u (C M + 3 |v|) with C = 44 (K <= 2.42: hfov <= 120 degrees;
             |offset| < |v| because R < focus).
  normalize3 v (1 / sqrt(dot3(v, v))): 3 u on the dot product (halved by the root), the root, the quotient, the product: 4.5 u of a
             unit vector.
  direction  |d_device - d_model| <= u (C M / |v| + C0),   C = 44, C0 = 7.5          — which is also the bound on the angle between them.
  origin     position + offset: the offset's 15.2 u R and the sum's own rounding, per component:
             |o_device - o_model|_inf <= C' u (|position|_inf + R),   C' = 17.        A pinhole's origin IS the position, bit for bit.
M / |v| is the cancellation: a camera far from the origin of the world that focuses close by subtracts large numbers to get a short
vector.  Nothing here was tuned on a device's output.  binary32 rounding of the model's own ray costs u per component and is inside
C0 and C'.
"""
import numpy as np

U = 2.0 ** -24
C_DIR, C0_DIR, C_ORIGIN = 44.0, 7.5, 17.0
UNCLEAR_BAND = 4.0 * 2.0 ** -23
WORLD_UP = np.array([0.0, 1.0, 0.0])


# ---- the random numbers, uint32 ---------------------------------------------------------------------

def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32)


def jenkins(x):
    x = np.array(x, dtype=np.uint32, ndmin=1)
    with np.errstate(over="ignore"):
        x = x + (x << np.uint32(10))
        x = x ^ (x >> np.uint32(6))
        x = x + (x << np.uint32(3))
        x = x ^ (x >> np.uint32(11))
        x = x + (x << np.uint32(15))
    return x


def seed(i, j, W, frame):
    with np.errstate(over="ignore"):
        s = (_u32(i) + _u32(j) * np.uint32(W)) ^ jenkins(_u32(frame))
    s = np.where(s == 0, np.uint32(1), s).astype(np.uint32)
    return jenkins(s)


def draw(s):
    """one xorshift step: (new state, value in [0, 1) as float64 — exact)"""
    s = s ^ (s << np.uint32(13))
    s = s ^ (s >> np.uint32(17))
    s = s ^ (s << np.uint32(5))
    return s, (s >> np.uint32(9)).astype(np.float64) * 2.0 ** -23


# ---- the camera -----------------------------------------------------------------------------------

class Camera:
    """the parameters, rounded to binary32 as the interface takes them, held as float64"""

    def __init__(self, position, forward, hfov_deg, W, H, focus=5.0, defocus_deg=0.0, name=""):
        self.position = np.asarray(position, np.float32).astype(np.float64)
        self.forward = np.asarray(forward, np.float32).astype(np.float64)
        self.hfov = float(np.float32(hfov_deg))
        self.focus = float(np.float32(focus))
        self.defocus = float(np.float32(defocus_deg))
        self.W, self.H = int(W), int(H)
        self.name = name

    def resized(self, W, H):
        return Camera(self.position, self.forward, self.hfov, W, H, self.focus, self.defocus, self.name)

    def args(self):
        """(position, forward, hfov, W, H, focus, defocus): the argument list of a camera constructor"""
        return tuple(self.position), tuple(self.forward), self.hfov, self.W, self.H, self.focus, self.defocus

    def basis(self, quirk=False):
        right = np.cross(self.forward, WORLD_UP)
        if not quirk:
            right = right / np.linalg.norm(right)
        return right, np.cross(right, self.forward)

    def half_width(self, hfov_scale=1.0):
        return self.focus * np.tan(np.radians(self.hfov * hfov_scale) / 2.0)

    def lens_radius(self, full_angle=False):
        return self.focus * np.tan(np.radians(self.defocus) / (1.0 if full_angle else 2.0))

    def struct(self, quirk=False):
        """what an nx_camera must hold, by name"""
        right, up = self.basis(quirk)
        a = self.half_width()
        vx, vy = 2.0 * a * right, 2.0 * a * self.H / self.W * up
        return dict(position=self.position, right=right, up=up, viewportX=vx, viewportY=vy,
                    lowerLeftCorner=self.position + self.focus * self.forward - vx / 2.0 - vy / 2.0, lensRadius=self.lens_radius(),
                    resolution=np.array([self.W, self.H]))

    def magnitude(self, quirk=False):
        """M of the bounds"""
        s = self.struct(quirk)
        right, _ = self.basis(quirk)
        return max(np.linalg.norm(s["lowerLeftCorner"]), np.linalg.norm(self.position), np.linalg.norm(s["viewportX"]), np.linalg.norm(s["viewportY"]),
                   self.lens_radius() * np.linalg.norm(right))

    def struct_bounds(self, quirk=False):
        """the host part of the bound, per field, as an absolute bound on every component (from the derivation above)"""
        s = self.struct(quirk)
        x = np.radians(self.hfov) / 2.0
        e_t = 2.0 * x / np.sin(2.0 * x) + 2.0
        M = self.magnitude(quirk)
        n = np.linalg.norm
        return dict(position=0.0, right=U * n(s["right"]), up=4.0 * U * n(s["up"]), viewportX=(e_t + 3.0) * U * n(s["viewportX"]), viewportY=(e_t + 8.0) * U * n(s["viewportY"]),
                    lowerLeftCorner=(e_t + 13.0) * U * M, lensRadius=4.1 * U * s["lensRadius"], resolution=0.0)


def _lens_draws(s, radial=False):
    """the rejection loop over a vector of states: (p (n, 2), unclear (n,)); radial: the disk from (r, phi) uniform in RADIUS — a wrong sampler"""
    n = len(s)
    p = np.zeros((n, 2))
    unclear = np.zeros(n, bool)
    if radial:
        s, a = draw(s)
        s, b = draw(s)
        return np.stack([a * np.cos(2.0 * np.pi * b), a * np.sin(2.0 * np.pi * b)], 1), unclear
    todo = np.arange(n)
    while len(todo):
        st, a = draw(s[todo])
        st, b = draw(st)
        s[todo] = st
        q = np.stack([2.0 * (a - 0.5), 2.0 * (b - 0.5)], 1)
        r2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]  # (exact: 24-bit numbers squared and added in 53 bits)
        unclear[todo] |= np.abs(r2 - 1.0) <= UNCLEAR_BAND
        ok = r2 < 1.0
        p[todo[ok]] = q[ok]
        todo = todo[~ok]
    return p, unclear


class Rays:
    pass


def primary_rays(cam, frame, pixels=None, quirk=False, variant=None):
    """The rays of global pixels `pixels` (default: all, in rows) of frame `frame`.  frame may be an array, one number per pixel.
    variant: a deliberately WRONG camera for the checker's self-tests and the transport controls —
      flip_v, swap_jitter, half_pixel, hfov_1001, lens_negated, lens_not_in_direction, tan_full_defocus, frame_plus_one, column_major,
      lens_radius_110, lens_radial."""
    W, H = cam.W, cam.H
    g = np.arange(W * H) if pixels is None else np.asarray(pixels, np.int64)
    if variant == "column_major":
        i, j = g // H, g % H
    else:
        i, j = g % W, g // W
    frame = np.broadcast_to(np.asarray(frame, np.int64), g.shape)
    s = seed(i, j, W, frame + (1 if variant == "frame_plus_one" else 0))
    s, jx = draw(s)
    s, jy = draw(s)
    if variant == "swap_jitter":
        jx, jy = jy, jx
    p, unclear = _lens_draws(s, radial=variant == "lens_radial")
    right, up = cam.basis(quirk)
    a = cam.half_width(1.001 if variant == "hfov_1001" else 1.0)
    b = a * H / W
    x = (i + jx + (0.5 if variant == "half_pixel" else 0.0)) / W
    y = (j + jy) / H
    if variant == "flip_v":
        y = 1.0 - y
    centre = cam.position + cam.focus * cam.forward
    F = centre + (2.0 * x - 1.0)[:, None] * a * right + (2.0 * y - 1.0)[:, None] * b * up
    R = cam.lens_radius(full_angle=variant == "tan_full_defocus") * (1.10 if variant == "lens_radius_110" else 1.0)
    offset = R * (p[:, 0:1] * right + p[:, 1:2] * up)
    if variant == "lens_negated":
        offset = -offset
    origin = cam.position + offset
    v = F - (cam.position if variant == "lens_not_in_direction" else origin)
    r = Rays()
    r.pixel, r.i, r.j, r.frame = g, i, j, frame
    r.jitter = np.stack([jx, jy], 1)
    r.lens, r.unclear = p, unclear
    r.focal, r.origin, r.v = F, origin, v
    r.direction = v / np.linalg.norm(v, axis=1, keepdims=True)
    r.offset = offset
    return r


def bounds(cam, rays, quirk=False):
    """(direction bound (n,), origin bound per component (scalar)) of the derivation in this file's docstring"""
    M = cam.magnitude(quirk)
    return U * (C_DIR * M / np.linalg.norm(rays.v, axis=1) + C0_DIR), C_ORIGIN * U * (np.max(np.abs(cam.position)) + cam.lens_radius())


def pixel_angle(cam, quirk=False):
    """the smaller of the two angular widths of every pixel, seen from the position through the pixel's centre lines: (W * H,)"""
    W, H = cam.W, cam.H
    g = np.arange(W * H)
    i, j = g % W, g // W
    right, up = cam.basis(quirk)
    a = cam.half_width()
    b = a * H / W

    def d(x, y):
        v = cam.focus * cam.forward + (2.0 * x / W - 1.0)[:, None] * a * right + (2.0 * y / H - 1.0)[:, None] * b * up
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def angle(p, q):
        return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.linalg.norm(p - q, axis=1)))

    return np.minimum(angle(d(i + 0.0, j + 0.5), d(i + 1.0, j + 0.5)), angle(d(i + 0.5, j + 0.0), d(i + 0.5, j + 1.0)))


def check_rays(cam, rays, origin, direction, quirk=False, unclear_cap=1e-4):
    """The ray checker: every clear path's origin and direction within the derived bound of the model's ray `rays`; a pinhole's origin
    equal to the position bit for bit; at most `unclear_cap` of the paths left out.  Returns a dict of what it saw; raises AssertionError
    with the worst path otherwise."""
    origin = np.asarray(origin)
    direction = np.asarray(direction)
    n = len(rays.pixel)
    assert origin.shape == (n, 3) and direction.shape == (n, 3), "the checker wants one ray per path"
    assert np.isfinite(origin).all() and np.isfinite(direction).all()
    clear = ~rays.unclear
    share = 1.0 - clear.sum() / n
    assert share <= unclear_cap, "%s: %.2e of the paths unclear" % (cam.name, share)
    bd, bo = bounds(cam, rays, quirk)
    ed = np.linalg.norm(direction.astype(np.float64) - rays.direction, axis=1)
    eo = np.max(np.abs(origin.astype(np.float64) - rays.origin), axis=1)
    rd = np.where(clear, ed / bd, 0.0)
    ro = np.where(clear, eo / bo, 0.0) if bo > 0 else np.where(clear & (eo > 0), np.inf, 0.0)
    k = int(np.argmax(rd))
    assert rd[k] <= 1.0, "%s: direction of path %d (pixel %d, %d frame %d) is %.3g from the model's, bound %.3g" % (cam.name, k, rays.i[k], rays.j[k], rays.frame[k], ed[k], bd[k])
    k = int(np.argmax(ro))
    assert ro[k] <= 1.0, "%s: origin of path %d (pixel %d, %d frame %d) is %.3g from the model's, bound %.3g" % (cam.name, k, rays.i[k], rays.j[k], rays.frame[k], eo[k], bo)
    if cam.defocus == 0.0:
        assert np.array_equal(np.asarray(origin, np.float32).view(np.uint32), np.broadcast_to(cam.position.astype(np.float32), (n, 3)).view(np.uint32)), \
            "%s: a pinhole's origin is the position, bit for bit" % cam.name
    return dict(unclear=share, worst_direction=float(rd.max()), worst_origin=float(ro.max()), paths=n)


def rejects(cam, rays, origin, direction, quirk=False):
    """True when check_rays refuses the rays (the self-tests' and the controls' question)"""
    try:
        check_rays(cam, rays, origin, direction, quirk)
    except AssertionError:
        return True
    return False


# ---- the cameras of the tests -----------------------------------------------------------------------------------
# (name, position, forward, hfov, focus, defocus, sizes).  Sizes are paired with cameras so that every bound stays under a thousandth of a
# pixel (test_bounds_meet_their_conditions); the short-focus camera stands near the world's origin for the same reason — the cancellation
# of a short focus far from the origin is what `far` is for, and `far` is held to its own bound only.

def _pitched(deg):
    t = np.radians(deg)
    return (0.0, float(np.sin(t)), float(-np.cos(t)))


CAMERAS = [
    ("level", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 60.0, 5.0, 0.0, [(64, 64), (33, 17), (1, 1)]),
    ("level_lens", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 60.0, 5.0, 10.0, [(64, 64), (33, 17)]),
    ("level_lens_small", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 60.0, 5.0, 0.5, [(33, 17), (7, 64)]),
    ("yawed", (0.0, 4.0, 14.0), (0.6, 0.0, -0.8), 60.0, 5.0, 10.0, [(33, 17), (7, 64)]),
    ("hfov5", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 5.0, 5.0, 0.5, [(7, 64), (1, 1)]),
    ("hfov120", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 120.0, 5.0, 10.0, [(130, 3), (33, 17)]),
    ("focus05", (0.0, 0.5, 1.0), (0.0, 0.0, -1.0), 60.0, 0.5, 10.0, [(33, 17), (7, 64)]),
    ("focus50", (0.0, 4.0, 14.0), (0.0, 0.0, -1.0), 60.0, 50.0, 0.5, [(64, 64), (130, 3)]),
    ("far", (1000.0, 4.0, 1000.0), (0.0, 0.0, -1.0), 60.0, 0.05, 10.0, [(33, 17)]),
    ("pitched_up", (0.0, 4.0, 14.0), _pitched(35.0), 60.0, 5.0, 10.0, [(33, 17), (7, 64)]),
    ("pitched_down", (0.0, 4.0, 14.0), _pitched(-35.0), 60.0, 5.0, 10.0, [(33, 17), (64, 64)]),
]
QUIRK = {"pitched_up", "pitched_down"}  # cameras whose forward is not level: right and up are cos(pitch) long in the code
FRAMES = (1, 2, 47)


def cameras():
    """every (Camera, quirk) of the table, one per size"""
    out = []
    for name, pos, fwd, hfov, focus, defocus, sizes in CAMERAS:
        for W, H in sizes:
            out.append((Camera(pos, fwd, hfov, W, H, focus, defocus, name="%s %dx%d" % (name, W, H)), name in QUIRK))
    return out


def camera(name, W, H):
    for n, pos, fwd, hfov, focus, defocus, _ in CAMERAS:
        if n == name:
            return Camera(pos, fwd, hfov, W, H, focus, defocus, name="%s %dx%d" % (name, W, H)), name in QUIRK
    raise KeyError(name)


# ---- depth of field as transport: the coverage of a half plane ---------------------------------------------------
# A level camera at the origin looks down -z; the plane z = -d is covered where x >= edge.  A ray from the lens point o through the
# focal point F (z = -focus) meets that plane at x = o.x + (F.x - o.x) d / focus: covered iff F.x >= (edge - o.x (1 - d / focus)) focus / d.

def coverage_model(cam, d, edge, radius_scale=1.0, radial=False, grid=600):
    """P(hit) per pixel COLUMN, by quadrature: F.x uniform over the column's cell (integrated in closed form), the lens point's
    x = R g(s) cos(phi) over a midpoint grid of (s, phi) in [0, 1)^2 — g = sqrt for the uniform disk, g = identity for the disk that is
    uniform in radius.  The integrand is continuous and piecewise linear in o.x: the midpoint rule's error falls as grid^-2."""
    a = cam.half_width()
    R = cam.lens_radius() * radius_scale
    m = (np.arange(grid) + 0.5) / grid
    s, phi = np.meshgrid(m, 2.0 * np.pi * m, indexing="ij")
    ox = (R * (s if radial else np.sqrt(s)) * np.cos(phi)).reshape(-1)
    need = (edge - ox * (1.0 - d / cam.focus)) * cam.focus / d  # F.x must be at least this
    x0 = -a + 2.0 * a * np.arange(cam.W) / cam.W
    x1 = x0 + 2.0 * a / cam.W
    return np.array([np.mean(np.clip((x1[c] - need) / (x1[c] - x0[c]), 0.0, 1.0)) for c in range(cam.W)])


def coverage_of_rays(rays, d, edge):
    """1.0 where the model's own ray meets the plane z = -d at x >= edge"""
    t = -d / rays.direction[:, 2]
    return ((rays.origin[:, 0] + t * rays.direction[:, 0]) >= edge).astype(np.float64)
