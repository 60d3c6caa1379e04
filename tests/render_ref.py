"""numpy restatement of the off-screen renderer's drawing rule, for the tests.

float32 for the projection (every operation rounded on its own: numpy never contracts), int64 for
the coverage, float64 for the camera and the colour.  Written from the rule's text and from the
reference's online_renderer.rs / draw.wgsl; it shares no code with csrc/nb_render.hip."""
import numpy as np

F = np.float32
HALF_SIZE = F(0.006)          # online_renderer.rs:224
CLEAR = (0.01, 0.0, 0.05)     # online_renderer.rs:345-349
ALPHA = 0.25                  # draw.wgsl:21
LIMIT = F(4194304.0)          # 2^22


# ---------------------------------------------------------------------------------------------
# camera (float64, rounded to float32 once)
# ---------------------------------------------------------------------------------------------
def default_camera(width, height):
    """online_renderer.rs:231-239.  aspect is the float32 quotient of the float32 sizes."""
    return dict(eye=(0.0, 1.0, 2.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
                aspect=float(F(width) / F(height)), fovy_deg=45.0, znear=float(F(0.00001)), zfar=100.0)


def view_proj64(cam):
    """OPENGL_TO_WGPU_MATRIX * perspective * look_at_rh (online_renderer.rs:41-54, cgmath's
    formulas) in float64 from the camera's float32 fields; returns the 4x4 matrix M[r, c]."""
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)  # noqa: E731
    eye, target, up = f32(cam["eye"]), f32(cam["target"]), f32(cam["up"])
    aspect, fovy, znear, zfar = (float(F(cam[k])) for k in ("aspect", "fovy_deg", "znear", "zfar"))
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731  (cgmath's order of the sums)
    cross = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2],  # noqa: E731
                                   a[0] * b[1] - a[1] * b[0]])
    f = target - eye
    f = f / np.sqrt(dot(f, f))
    s = cross(f, up)
    s = s / np.sqrt(dot(s, s))
    u = cross(s, f)
    view = [[s[0], s[1], s[2], -dot(s, eye)],
            [u[0], u[1], u[2], -dot(u, eye)],
            [-f[0], -f[1], -f[2], dot(f, eye)],
            [0.0, 0.0, 0.0, 1.0]]
    c = 1.0 / np.tan(fovy * (np.pi / 180.0) / 2.0)
    proj = [[c / aspect, 0.0, 0.0, 0.0],
            [0.0, c, 0.0, 0.0],
            [0.0, 0.0, (zfar + znear) / (znear - zfar), 2.0 * zfar * znear / (znear - zfar)],
            [0.0, 0.0, -1.0, 0.0]]
    gl2wgpu = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0]]

    def matmul(a, b):  # sums in the order k = 0, 1, 2, 3 from 0.0, as a plain loop does
        out = np.zeros((4, 4))
        for r in range(4):
            for col in range(4):
                acc = 0.0
                for k in range(4):
                    acc += a[r][k] * b[k][col]
                out[r, col] = acc
        return out

    return matmul(gl2wgpu, matmul(proj, view))


def view_proj(cam):
    """The 16 floats, column-major: out[4 c + r] = M[r, c]."""
    return np.ascontiguousarray(view_proj64(cam).T.reshape(16).astype(np.float32))


# ---------------------------------------------------------------------------------------------
# projection and snapping (float32)
# ---------------------------------------------------------------------------------------------
def project(xyz, vp, width, height, half_size=HALF_SIZE):
    """xyz: float32 [n, 3].  Returns (tri, cls): tri int64 [n, 3, 2] snapped vertices (valid where
    cls == 0), cls: 0 drawn, 1 clipped, 2 oversize, 3 nonfinite."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    vp = np.asarray(vp, dtype=np.float32).reshape(16)
    n = xyz.shape[0]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    s = F(half_size)
    wf, hf, half = F(width), F(height), F(0.5)
    with np.errstate(all="ignore"):
        cx, cy, cz, cw = [((vp[r] * x + vp[4 + r] * y) + vp[8 + r] * z) + vp[12 + r] for r in range(4)]
        nonfinite = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
        visible = (cw > 0) & (cz >= 0) & (cz <= cw)
        tri = np.zeros((n, 3, 2), dtype=np.int64)
        inside = np.ones(n, dtype=bool)
        for k, (ox, oy) in enumerate(((-s, -s), (s, -s), (F(0.0), s))):
            nx = (cx + ox) / cw
            ny = (cy + oy) / cw
            sx = (nx * half + half) * wf
            sy = (half - ny * half) * hf
            # "any |s| >= 2^22 is oversize": a NaN (inf/inf of an overflowed product) is not below
            # the limit either
            ok = (np.abs(sx) < LIMIT) & (np.abs(sy) < LIMIT)
            inside &= ok
            tri[:, k, 0] = np.rint(np.where(ok, sx, F(0)) * F(256.0)).astype(np.int64)
            tri[:, k, 1] = np.rint(np.where(ok, sy, F(0)) * F(256.0)).astype(np.int64)
    cls = np.where(nonfinite, 3, np.where(~visible, 1, np.where(~inside, 2, 0))).astype(np.int32)
    return tri, cls


# ---------------------------------------------------------------------------------------------
# coverage (int64)
# ---------------------------------------------------------------------------------------------
def cover(tri, x0, y0, bw, bh):
    """Coverage of the snapped triangles tri [m, 3, 2] over pixel windows of bw x bh pixels whose
    first pixel is (x0[t], y0[t]): bool [m, bh, bw].  Pixel (i, j) has its centre at (256 i + 128,
    256 j + 128); integer edge functions, either winding, top-left rule, zero area covers nothing."""
    tri = np.asarray(tri, dtype=np.int64)
    m = tri.shape[0]
    ax, ay = tri[:, 0, 0], tri[:, 0, 1]
    area = (tri[:, 1, 0] - ax) * (tri[:, 2, 1] - ay) - (tri[:, 1, 1] - ay) * (tri[:, 2, 0] - ax)
    g = np.sign(area)
    px = (256 * (np.asarray(x0, dtype=np.int64)[:, None] + np.arange(bw, dtype=np.int64)[None, :]) + 128)[:, None, :]
    py = (256 * (np.asarray(y0, dtype=np.int64)[:, None] + np.arange(bh, dtype=np.int64)[None, :]) + 128)[:, :, None]
    cov = np.broadcast_to((g != 0)[:, None, None], (m, bh, bw)).copy()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        vax, vay = tri[:, a, 0][:, None, None], tri[:, a, 1][:, None, None]
        ex, ey = tri[:, b, 0] - tri[:, a, 0], tri[:, b, 1] - tri[:, a, 1]
        e = g[:, None, None] * (ex[:, None, None] * (py - vay) - ey[:, None, None] * (px - vax))
        topleft = (g * ey < 0) | ((ey == 0) & (g * ex > 0))
        cov &= (e > 0) | ((e == 0) & topleft[:, None, None])
    return cov


def rasterize(tri, width, height, per_triangle=False):
    """counts uint32 [height, width] of snapped triangles tri int64 [m, 3, 2], scissored to the
    image.  per_triangle: also the number of image pixels each one covers."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3, 2)
    m = tri.shape[0]
    counts = np.zeros((height, width), dtype=np.int64)
    flat = counts.reshape(-1)
    per = np.zeros(m, dtype=np.int64)
    if m:
        # first and last pixel whose centre lies within the bounding box, cut to the image
        lo = np.maximum(-((128 - tri.min(axis=1)) // 256), 0)                 # ceil((min - 128) / 256)
        hi = np.minimum((tri.max(axis=1) - 128) // 256, np.array([width - 1, height - 1]))
        ext = hi - lo + 1
        size = np.where((ext > 0).all(axis=1), ext.max(axis=1), 0)
        below = 0
        for cap in (4, 8, 16, 64):                                            # square windows, by size class
            sel = np.nonzero((size > below) & (size <= cap))[0]
            below = cap
            chunk = max(1, (1 << 22) // (cap * cap))
            for s0 in range(0, sel.size, chunk):
                idx = sel[s0:s0 + chunk]
                cov = cover(tri[idx], lo[idx, 0], lo[idx, 1], cap, cap)
                ii = lo[idx, 0][:, None, None] + np.arange(cap)[None, None, :]
                jj = lo[idx, 1][:, None, None] + np.arange(cap)[None, :, None]
                cov &= (ii <= hi[idx, 0][:, None, None]) & (jj <= hi[idx, 1][:, None, None])
                per[idx] = cov.sum(axis=(1, 2))
                np.add.at(flat, (jj * width + ii)[cov], 1)
        for t in np.nonzero(size > 64)[0]:                                    # large: one at a time, in bands
            for r0 in range(int(lo[t, 1]), int(hi[t, 1]) + 1, 128):
                rows = min(128, int(hi[t, 1]) + 1 - r0)
                cov = cover(tri[t:t + 1], lo[t:t + 1, 0], np.array([r0]), int(ext[t, 0]), rows)[0]
                per[t] += cov.sum()
                counts[r0:r0 + rows, lo[t, 0]:hi[t, 0] + 1] += cov
    out = counts.astype(np.uint32)
    return (out, per) if per_triangle else out


# ---------------------------------------------------------------------------------------------
# the whole rule
# ---------------------------------------------------------------------------------------------
def render_counts(xyz, vp, width, height, half_size=HALF_SIZE):
    """counts uint32 [H, W] and the stats dict of the drawing rule."""
    tri, cls = project(xyz, vp, width, height, half_size)
    counts = rasterize(tri[cls == 0], width, height)
    stats = dict(n=int(cls.size), drawn=int((cls == 0).sum()), clipped=int((cls == 1).sum()),
                 oversize=int((cls == 2).sum()), nonfinite=int((cls == 3).sum()),
                 fragments=int(counts.sum(dtype=np.uint64)), max_count=int(counts.max()) if counts.size else 0)
    return counts, stats


def srgb_encode(lin):
    lin = np.asarray(lin, dtype=np.float64)
    return np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(np.maximum(lin, 0.0), 1.0 / 2.4) - 0.055)


def colour64(counts, clear=CLEAR, alpha=ALPHA, srgb=True):
    """float64 closed form before the rounding to bytes: 255 enc(1 - (1 - clear)(1 - alpha)^k),
    shape counts.shape + (3,), from the float32 clear and alpha the device is given."""
    k = np.asarray(counts).astype(np.float64)[..., None]
    clear = np.asarray([float(F(c)) for c in clear])
    lin = 1.0 - (1.0 - clear) * np.power(1.0 - float(F(alpha)), k)
    return 255.0 * (srgb_encode(lin) if srgb else lin)


def rgba8(counts, clear=CLEAR, alpha=ALPHA, srgb=True):
    c = np.asarray(counts)
    out = np.full(c.shape + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.clip(np.rint(colour64(c, clear, alpha, srgb)), 0, 255).astype(np.uint8)
    return out


def read_ppm(path):
    """A binary P6 file with maxval 255 -> uint8 [H, W, 3]."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:3] == b"P6\n", data[:16]
    head, rest = data[3:].split(b"\n", 1)
    w, h = (int(v) for v in head.split())
    maxval, body = rest.split(b"\n", 1)
    assert int(maxval) == 255 and len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)
