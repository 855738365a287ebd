"""The case list of the YUV tests: sizes, pitches, row counts and contents.  What each is for:

  sizes    2 x 2 one lane with one pixel pair; 6 x 4 fewer than a lane's 8 pixels; 14 x 2, 18 x 6, 30 x 10 row tails of 6, 2
           and 6 pixels behind 1, 2 and 3 full lanes (250 x 130: a tail of 2 behind 31 lanes, 66 x 34: of 2); 1022 x 4 a
           tail of 6 and 1026 x 6 one pixel pair past the 512-pixel row of two waves; h = 2: a single block row
  pitches  tight, + 2 (no aligned access anywhere), + 62, rounded up to 256 (a decoder's), and an odd one for the
           layouts that may have it
  rows     h, h + 2, h + 6: where the chroma area and the next frame start
  contents uniform noise saturates a channel for 84 % of its triples, so it comes with "legal" frames (the encode of
           random RGB), the extremes of the three ranges, and for the encode the corners of the RGB cube and blocks
           whose four pixels differ strongly (a mean in place of the top-left sample cannot pass)
"""
import numpy as np

import yuv_ref as yr

SIZES = [(2, 2), (6, 4), (14, 2), (18, 6), (30, 10), (66, 34), (250, 130), (1022, 4), (1026, 6)]
ROW_EXTRAS = (0, 2, 6)
Y_EXTREMES = (0, 15, 16, 17, 234, 235, 236, 255)
C_EXTREMES = (0, 1, 127, 128, 129, 255)
CUBE = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def _up(x, m):
    return (x + m - 1) // m * m


def pitches(layout, w):
    """the pitches of a layout at width w, in bytes"""
    tight = 2 * w if yr.is_packed(layout) else w
    out = [tight, tight + 2, tight + 62, _up(tight, 256)]
    if not yr.is_planar(layout):
        out.append(tight + 3)
    return out


def geometries(layout, w, h):
    """every (pitch, rows) of the list for a layout and a size"""
    return [(p, h + e) for p in pitches(layout, w) for e in ROW_EXTRAS]


def _chroma_shape(w, h, packed):
    return (h, w // 2) if packed else (h // 2, w // 2)


def noise_planes(w, h, packed, seed):
    rng = np.random.default_rng(seed)
    cs = _chroma_shape(w, h, packed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, cs, dtype=np.uint8),
            rng.integers(0, 256, cs, dtype=np.uint8))


def legal_planes(w, h, packed, seed):
    """the encode of random RGB: triples a real picture holds, which mostly do not saturate"""
    rgba = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    return yr.encode_planes(rgba, yr.BT601, packed)


def extreme_planes(w, h, packed, seed):
    """every (Y, U, V) of Y_EXTREMES x C_EXTREMES^2, as far as the frame has room, starting at combination `seed`"""
    cs = _chroma_shape(w, h, packed)
    i = (np.arange(cs[0] * cs[1]).reshape(cs) + seed) % (len(C_EXTREMES) ** 2)
    u = np.array(C_EXTREMES, np.uint8)[i // len(C_EXTREMES)]
    v = np.array(C_EXTREMES, np.uint8)[i % len(C_EXTREMES)]
    yy, xx = np.mgrid[0:h, 0:w]
    block = (yy // (1 if packed else 2)) * cs[1] + xx // 2 + seed
    y = np.array(Y_EXTREMES, np.uint8)[(block // (len(C_EXTREMES) ** 2) + (xx % 2) + 2 * (yy % 2)) % len(Y_EXTREMES)]
    return y, u, v


def decode_contents(w, h, packed):
    """[(name, (Y, U, V))]: the three contents of a decode or luma case"""
    seed = w * 1000 + h
    return [("noise", noise_planes(w, h, packed, seed)), ("legal", legal_planes(w, h, packed, seed + 1)),
            ("extremes", extreme_planes(w, h, packed, seed))]


def cube_rgba(w, h, seed):
    """RGB noise (alpha too: it is ignored) with the corners of the cube on top-left pixels of blocks"""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    bw = w // 2
    for k in range(min(len(CUBE), bw * (h // 2))):
        a[2 * (k // bw), 2 * (k % bw), :3] = CUBE[(k + seed) % len(CUBE)]
    return a


def blocks_rgba(w, h, seed):
    """each 2 x 2 block: a random top-left pixel, its complement to the right, and two other far pixels below"""
    rng = np.random.default_rng(seed)
    a = np.empty((h, w, 4), np.uint8)
    tl = rng.integers(0, 256, (h // 2, w // 2, 4), dtype=np.uint8)
    a[0::2, 0::2] = tl
    a[0::2, 1::2] = 255 - tl
    a[1::2, 0::2] = tl ^ 0x80
    a[1::2, 1::2] = (255 - tl) ^ 0x55
    return a


def encode_contents(w, h):
    """[(name, rgba)]: the two contents of an encode case"""
    seed = w * 1000 + h
    return [("cube", cube_rgba(w, h, seed)), ("blocks", blocks_rgba(w, h, seed + 1))]


def padding(nbytes, seed):
    """arbitrary bytes for the padding of a pitched frame (or a whole batch)"""
    return np.random.default_rng(seed ^ 0x9E37).integers(0, 256, nbytes, dtype=np.uint8)


def pack_batch(contents, layout, pitch, rows, seed=7):
    """the frames of `contents` ([(name, planes)]) back to back, padding filled with arbitrary bytes"""
    h, w = contents[0][1][0].shape
    fb = yr.frame_bytes(layout, w, h, pitch, rows)
    fill = padding(fb * len(contents), seed).reshape(len(contents), fb)
    return np.concatenate([yr.pack(p, layout, pitch, rows, fill[i]) for i, (_, p) in enumerate(contents)])
