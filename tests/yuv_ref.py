"""CPU reference of the YUV calls (mi355_yuv_*): a plain numpy restatement of the header text, int64 inside.

Written from include/mi355_imgfilter.h ("frames from a decoder or a camera"), not from the kernel: the byte positions of
every layout, the two formulas and the table of constants.  Planes are what the formulas speak of:
  4:2:0   Y (h, w), U and V (h / 2, w / 2)
  packed  Y (h, w), U and V (h, w / 2)
pack() / unpack() move planes into and out of one frame's bytes for a layout, a pitch and a row count.
"""
import numpy as np

NV12, NV21, I420, YV12, YUY2, UYVY = range(6)
LAYOUTS = (NV12, NV21, I420, YV12, YUY2, UYVY)
LAYOUT_NAMES = ("nv12", "nv21", "i420", "yv12", "yuy2", "uyvy")
BT601, BT709, BT601_FULL = range(3)
STANDARDS = (BT601, BT709, BT601_FULL)

# the header's table: YOFF CY CVR CVG CUG CUB / CRY CGY CBY CRU CGU CBU CGV CBV
DECODE = {
    BT601: dict(YOFF=16, CY=1220542, CVR=1673527, CVG=-852492, CUG=-409993, CUB=2116026),
    BT709: dict(YOFF=16, CY=1220945, CVR=1879825, CVG=-558796, CUG=-223607, CUB=2215014),
    BT601_FULL: dict(YOFF=0, CY=1048576, CVR=1470104, CVG=-748826, CUG=-360853, CUB=1858077),
}
ENCODE = {
    BT601: dict(YOFF=16, CRY=269484, CGY=528482, CBY=102760, CRU=-155188, CGU=-305135, CBU=460324, CGV=-385875,
                CBV=-74448),
    BT709: dict(YOFF=16, CRY=191455, CGY=644067, CBY=65019, CRU=-105533, CGU=-355018, CBU=460551, CGV=-418321,
                CBV=-42230),
    BT601_FULL: dict(YOFF=0, CRY=313524, CGY=615514, CBY=119538, CRU=-176932, CGU=-347356, CBU=524288, CGV=-439026,
                     CBV=-85262),
}
HALF = 1 << 19


def is_packed(layout):
    return layout in (YUY2, UYVY)


def is_planar(layout):
    return layout in (I420, YV12)


def resolve(layout, w, h, pitch=0, rows=0):
    """(pitch, rows) with the zeros replaced: tight rows, h rows"""
    return (pitch or (2 * w if is_packed(layout) else w)), (rows or h)


def accepted(layout, w, h, pitch=0, rows=0):
    """the geometry rules of the header (sizes themselves aside)"""
    if layout not in LAYOUTS or w <= 0 or h <= 0 or w % 2 or pitch < 0 or rows < 0:
        return False
    p, r = resolve(layout, w, h, pitch, rows)
    if p < (2 * w if is_packed(layout) else w) or r < h:
        return False
    if not is_packed(layout) and (h % 2 or r % 2):
        return False
    return not (is_planar(layout) and p % 2)


def frame_bytes(layout, w, h, pitch=0, rows=0):
    if not accepted(layout, w, h, pitch, rows):
        return 0
    p, r = resolve(layout, w, h, pitch, rows)
    return p * r if is_packed(layout) else p * r * 3 // 2


def _positions(layout, w, h, pitch, rows):
    """byte offsets in a frame of (Y, U, V), each with the shape of its plane"""
    p, r = resolve(layout, w, h, pitch, rows)
    yy, xx = np.mgrid[0:h, 0:w]
    if is_packed(layout):
        cy, cx = np.mgrid[0:h, 0:w // 2]
        pair = cy * p + 4 * cx                   # Y0 U Y1 V (YUY2) or U Y0 V Y1 (UYVY)
        if layout == YUY2:
            return yy * p + 2 * xx, pair + 1, pair + 3
        return yy * p + 2 * xx + 1, pair, pair + 2
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    ypos = yy * p + xx
    if layout in (NV12, NV21):
        first = r * p + cy * p + 2 * cx
        second = first + 1
    else:
        first = r * p + cy * (p // 2) + cx
        second = first + (p // 2) * (r // 2)
    return (ypos, first, second) if layout in (NV12, I420) else (ypos, second, first)


def pixel_mask(layout, w, h, pitch=0, rows=0):
    """True for the bytes of a frame that belong to a pixel, False for padding"""
    m = np.zeros(frame_bytes(layout, w, h, pitch, rows), bool)
    for pos in _positions(layout, w, h, pitch, rows):
        m[pos.ravel()] = True
    return m


def pack(planes, layout, pitch=0, rows=0, fill=0):
    """One frame's bytes from (Y, U, V).  fill: what the padding holds, a byte value or an array of frame_bytes bytes."""
    y, u, v = (np.asarray(a, np.uint8) for a in planes)
    h, w = y.shape
    assert u.shape == v.shape == ((h, w // 2) if is_packed(layout) else (h // 2, w // 2))
    n = frame_bytes(layout, w, h, pitch, rows)
    assert n, "geometry not accepted"
    out = np.full(n, fill, np.uint8) if np.isscalar(fill) else np.array(fill, np.uint8).reshape(n).copy()
    for pos, plane in zip(_positions(layout, w, h, pitch, rows), (y, u, v)):
        out[pos.ravel()] = plane.ravel()
    return out


def unpack(frame, layout, w, h, pitch=0, rows=0):
    frame = np.asarray(frame, np.uint8).ravel()
    assert frame.size == frame_bytes(layout, w, h, pitch, rows)
    return tuple(frame[pos] for pos in _positions(layout, w, h, pitch, rows))


def _sat(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def decode_planes(y, u, v, standard=BT601):
    """(h, w, 4) RGBA of planes; U and V (h / 2 or h, w / 2) serve every pixel of their block or pair"""
    c = DECODE[standard]
    h, w = y.shape
    u = np.repeat(u, 2, axis=1)
    v = np.repeat(v, 2, axis=1)
    if u.shape[0] != h:
        u, v = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)
    uu, vv = u.astype(np.int64) - 128, v.astype(np.int64) - 128
    yy = np.maximum(0, y.astype(np.int64) - c["YOFF"]) * c["CY"]
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0] = _sat((yy + HALF + c["CVR"] * vv) >> 20)
    out[..., 1] = _sat((yy + HALF + c["CVG"] * vv + c["CUG"] * uu) >> 20)
    out[..., 2] = _sat((yy + HALF + c["CUB"] * uu) >> 20)
    out[..., 3] = 255
    return out


def _frames_of(buf, nbytes):
    buf = np.asarray(buf, np.uint8).ravel()
    assert nbytes and buf.size % nbytes == 0
    return buf.reshape(-1, nbytes)


def decode(buf, w, h, layout, standard=BT601, pitch=0, rows=0):
    """(n, h, w, 4) RGBA of n frames back to back in buf"""
    frames = _frames_of(buf, frame_bytes(layout, w, h, pitch, rows))
    return np.stack([decode_planes(*unpack(f, layout, w, h, pitch, rows), standard) for f in frames])


def luma(buf, w, h, layout, pitch=0, rows=0):
    """(n, h, w): the Y bytes, unchanged"""
    frames = _frames_of(buf, frame_bytes(layout, w, h, pitch, rows))
    return np.stack([unpack(f, layout, w, h, pitch, rows)[0] for f in frames])


def encode_planes(rgba, standard=BT601, packed=False):
    """(Y, U, V) of one (h, w, 4) frame.  U and V come from the top-left pixel of each 2 x 2 block; with `packed` (no call
    encodes that; it makes legal test content) from the left pixel of each pair."""
    c = ENCODE[standard]
    a = np.asarray(rgba, np.uint8).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = _sat((c["CRY"] * r + c["CGY"] * g + c["CBY"] * b + HALF + (c["YOFF"] << 20)) >> 20)
    sub = (slice(None), slice(None, None, 2)) if packed else (slice(None, None, 2), slice(None, None, 2))
    r, g, b = r[sub], g[sub], b[sub]
    u = _sat((c["CRU"] * r + c["CGU"] * g + c["CBU"] * b + HALF + (128 << 20)) >> 20)
    v = _sat((c["CBU"] * r + c["CGV"] * g + c["CBV"] * b + HALF + (128 << 20)) >> 20)
    return y, u, v


def encode(rgba, layout, standard=BT601, pitch=0, rows=0, fill=0):
    """(n, frame bytes) of (n, h, w, 4) or (h, w, 4) RGBA; fill as in pack(), per frame when it is an array of n rows"""
    assert not is_packed(layout), "the encode is offered for the 4:2:0 layouts"
    a = np.asarray(rgba, np.uint8)
    a = a[None] if a.ndim == 3 else a
    fills = [fill] * len(a) if np.isscalar(fill) else list(np.asarray(fill, np.uint8).reshape(len(a), -1))
    return np.stack([pack(encode_planes(f, standard), layout, pitch, rows, fl) for f, fl in zip(a, fills)])
