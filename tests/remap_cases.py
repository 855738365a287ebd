"""The shapes, maps and homographies the remap tests share (tests/test_remap_cpu.py checks on the reference's coordinates
that each of them reaches the case it is there for; tests/test_gpu_remap.py runs them on the GPU).  A plain helper module.
"""
import numpy as np

from remap_ref import FIXED, FLOAT, convert_maps
from warp_ref import INVERSE_MAP, LINEAR, NEAREST, fixed_coords, inverse_of, rotation

# The kernel's tile, restated from csrc/kernels.hpp (kRemapLanesLog2 = 3 lanes of 4 pixels, kRemapTileH rows): one wave
# owns a tile across kRemapFrames frames and votes once per row pass of 64 >> kRemapLanesLog2 rows.
TILE, LANE_ROWS, FRAMES_PER_ITEM = (32, 32), 8, 4

# (src w, src h, dst w, dst h): one pixel, fewer columns than a lane owns, ragged last lanes and tiles, more than one tile
# in each direction, a wide flat and a tall thin frame; then a dst one tile wide plus 1, two tiles high plus 1, one tile.
SHAPES = [(1, 1, 1, 1), (5, 3, 7, 2), (64, 48, 21, 16), (77, 41, 130, 19), (1023, 9, 640, 5), (3, 1000, 5, 700),
          (80, 50, TILE[0] + 1, 7), (50, 80, 9, 2 * TILE[1] + 1), (100, 60, TILE[0], TILE[1])]
VALUES = (0, 0x80FF407F)


def pack_fixed(sx, sy, fx, fy):
    """FIXED maps from int64 coordinate arrays (they must fit a short)."""
    assert sx.min() >= -32768 and sx.max() <= 32767 and sy.min() >= -32768 and sy.max() <= 32767
    return np.stack([sx, sy], -1).astype(np.int16), (fy * 32 + fx).astype(np.uint16)


def affine_fixed_maps(m, dw, dh, flags, rows=None):
    """FIXED maps holding exactly the (sx, sy, fx, fy) warp_ref takes for the affine matrix m."""
    X, Y = fixed_coords(m, dw, dh, flags, rows)
    if (flags & ~INVERSE_MAP) == NEAREST:
        return pack_fixed(X >> 10, Y >> 10, np.zeros_like(X), np.zeros_like(X))
    X, Y = X >> 5, Y >> 5
    return pack_fixed(X >> 5, Y >> 5, X & 31, Y & 31)


def affine_float_maps(m, dw, dh, flags=0):
    """FLOAT maps of the affine matrix m: the source position in fp64, rounded once to float32."""
    i = inverse_of(m, flags)
    x, y = np.arange(dw, dtype=np.float64)[None, :], np.arange(dh, dtype=np.float64)[:, None]
    return (i[0] * x + i[1] * y + i[2]).astype(np.float32), (i[3] * x + i[4] * y + i[5]).astype(np.float32)


def identity_float_maps(dw, dh):
    return affine_float_maps([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dw, dh, INVERSE_MAP)


def barrel_float_maps(sw, sh, dw, dh, rows=None):
    """r' = r (1 + 0.2 r^2) about the centre, r = 1 at the middle of an edge: the corners sample outside the source."""
    ys = np.arange(dh) if rows is None else np.asarray(rows)
    nx = ((np.arange(dw, dtype=np.float64) - (dw - 1) / 2.0) / (dw / 2.0))[None, :]
    ny = ((ys.astype(np.float64) - (dh - 1) / 2.0) / (dh / 2.0))[:, None]
    k = 1.0 + 0.2 * (nx * nx + ny * ny)
    return (((sw - 1) / 2.0 + nx * k * (sw / 2.0)).astype(np.float32),
            ((sh - 1) / 2.0 + ny * k * (sh / 2.0)).astype(np.float32))


def outside_float_maps(dw, dh):
    return np.full((dh, dw), 5000.0, np.float32), np.full((dh, dw), 5000.0, np.float32)


SPECIAL_FLOATS = ("nan", "+inf", "-inf", "+3e9", "-3e9", "seam")


def special_float_maps(sw, sh, dw, dh):
    """Identity maps with the special values planted one after the other from entry 0 on (fewer where the map is
    smaller), x and y alike except the seam, which is sw - 0.5 in x only.  Returns (map_x, map_y, {name: flat index})."""
    mx, my = identity_float_maps(dw, dh)
    vals = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+3e9": 3.0e9, "-3e9": -3.0e9}
    at = {}
    for k, name in enumerate(SPECIAL_FLOATS):
        if k >= dw * dh:
            break
        y, x = divmod(k, dw)
        if name == "seam":
            mx[y, x], my[y, x] = sw - 0.5, 0.0
        else:
            mx[y, x] = my[y, x] = vals[name]
        at[name] = k
    return mx, my, at


SPECIAL_FIXED = ("-32768", "32767", "seam", "map2>1023", "map2=65535")


def special_fixed_maps(sw, sh, dw, dh):
    """Identity FIXED maps with the special entries planted from entry 0 on: sx = sy = -32768, sx = sy = 32767,
    sx = sw - 1 with fx = 16, and map2 entries above 1023 whose high bits must be ignored (1024 + 5 -> fx 5, fy 0;
    65535 -> fx = fy = 31).  Returns (map1, map2, {name: flat index})."""
    x, y = np.meshgrid(np.arange(dw), np.arange(dh))
    map1 = np.stack([x, y], -1).astype(np.int16)
    map2 = np.zeros((dh, dw), np.uint16)
    entries = {"-32768": ((-32768, -32768), 0), "32767": ((32767, 32767), 7 * 32 + 9), "seam": ((sw - 1, 0), 16),
               "map2>1023": ((0, 0), 1024 + 5), "map2=65535": ((0, 0), 65535)}
    at = {}
    for k, name in enumerate(SPECIAL_FIXED):
        if k >= dw * dh:
            break
        yy, xx = divmod(k, dw)
        map1[yy, xx], map2[yy, xx] = entries[name]
        at[name] = k
    return map1, map2, at


def remap_maps(sw, sh, dw, dh, map_kind, interp):
    """[(name, map1, map2)] of a shape for one map kind: identity, the rot30 affine map, the barrel distortion,
    all-outside and the special values."""
    rot30 = rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)
    if map_kind == FLOAT:
        return [("identity",) + identity_float_maps(dw, dh), ("rot30",) + affine_float_maps(rot30, dw, dh),
                ("barrel",) + barrel_float_maps(sw, sh, dw, dh), ("outside",) + outside_float_maps(dw, dh),
                ("special",) + special_float_maps(sw, sh, dw, dh)[:2]]
    assert map_kind == FIXED
    return [("identity",) + convert_maps(*identity_float_maps(dw, dh), interp),
            ("rot30",) + affine_fixed_maps(rot30, dw, dh, interp),
            ("barrel",) + convert_maps(*barrel_float_maps(sw, sh, dw, dh), interp),
            ("outside",) + convert_maps(*outside_float_maps(dw, dh), interp),
            ("special",) + special_fixed_maps(sw, sh, dw, dh)[:2]]


W_ZERO = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -5.0]         # inverse-mapped: w = x - 5, exactly 0 on column 5
W_SIGN = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.3, 0.0, 1.0]         # inverse-mapped: w = 1 - 0.3 x changes sign after column 3
KEYSTONE = [1.0, 0.1, -3.0, 0.02, 1.05, -2.0, 1.0e-3, -1.0e-3, 1.0]


def embed(m6):
    """A 2 x 3 affine matrix as a homography with last row (0, 0, 1)."""
    return [float(v) for v in m6] + [0.0, 0.0, 1.0]


def homographies(sw, sh):
    """The eight matrices of a source shape; each runs inverse-mapped and forward."""
    return [("identity", embed([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])),
            ("shift+3-2", embed([1.0, 0.0, 3.0, 0.0, 1.0, -2.0])),
            ("rot30", embed(rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0))),
            ("keystone", KEYSTONE), ("w==0", W_ZERO), ("w-sign", W_SIGN),
            ("singular", [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 1.0, 1.0, 1.0]),
            ("outside", embed([1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0]))]


def keystone_4k(sw, sh):
    """A keystone for large frames: the top edge keeps its width, the bottom edge is squeezed by about a quarter."""
    return [1.0, 0.12, -40.0, 0.0, 1.1, -25.0, 0.0, 1.2e-4, 1.0]
