"""The statement "Word strips"  in plain Python loops over Python integers: what csrc/word_strips.hip and the host path of
qea/reading.py reproduce bit for bit.  Nothing here is shared with either."""
import numpy as np

OH = 32


def norm():
    """float32(p) / 255 for the 256 byte values: one fp32 division each"""
    return (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)


def quantise(page):
    """the 8-bit value of a float pixel: (uint8)(min(max(x, 0), 1) * 255) in fp32, truncated, NaN -> 0"""
    x = np.asarray(page, np.float32)
    x = np.where(x != x, np.float32(0), x)
    return (np.minimum(np.maximum(x, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8)


def floordiv2(d):
    return d // 2                                            # Python floors: -3 // 2 == -2


def clip(box, sizes):
    """(page, x0, y0, x1, y1), exclusive, and the pages' (h, w) list -> (page, x0, y0, cw, ch), or None for a white strip"""
    p, x0, y0, x1, y1 = (int(v) for v in box)
    if p < 0 or p >= len(sizes):
        return None
    h, w = sizes[p]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    cw, ch = x1 - x0, y1 - y0
    if cw <= 0 or ch <= 0:
        return None
    return p, x0, y0, cw, ch


def scaled_width(cw, ch):
    return cw if ch <= OH else (32 * cw + ch - 1) // ch


def overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def area_pixel(page, x0, y0, cw, ch, oy, j):
    """-> (q, S, Area, [(r, c, wy, wx)]) of scaled pixel (row oy, column j) of a box with ch > 32, lengths in 1 / 32 source pixel"""
    ya, yb = oy * ch, (oy + 1) * ch
    xa, xb = j * ch, min((j + 1) * ch, 32 * cw)
    S, taps = 0, []
    for r in range(ch):
        wy = overlap(ya, yb, 32 * r, 32 * r + 32)
        if not wy:
            continue
        for c in range(cw):
            wx = overlap(xa, xb, 32 * c, 32 * c + 32)
            if wx:
                S += wy * wx * int(page[y0 + r][x0 + c])
                taps.append((r, c, wy, wx))
    area = ch * min(ch, 32 * cw - j * ch)
    assert area == (yb - ya) * (xb - xa) == sum(wy * wx for _, _, wy, wx in taps)
    q = (2 * S + area) // (2 * area)
    assert 0 <= q <= 255
    return q, S, area, taps


def levels(page, x0, y0, cw, ch):
    """the 8-bit strip content before placement: [rows][cols] with rows = min(ch, 32), cols = scaled_width"""
    if ch <= OH:
        return [[int(page[y0 + r][x0 + c]) for c in range(cw)] for r in range(ch)]
    sw = scaled_width(cw, ch)
    # the taps of a pixel are a contiguous range of rows and columns: walk only those (area_pixel above walks them all)
    out = []
    for oy in range(OH):
        ya, yb = oy * ch, (oy + 1) * ch
        row = []
        for j in range(sw):
            xa, xb = j * ch, min((j + 1) * ch, 32 * cw)
            S = 0
            for r in range(ya // 32, (yb - 1) // 32 + 1):
                wy = overlap(ya, yb, 32 * r, 32 * r + 32)
                for c in range(xa // 32, (xb - 1) // 32 + 1):
                    S += wy * overlap(xa, xb, 32 * c, 32 * c + 32) * int(page[y0 + r][x0 + c])
            area = ch * (xb - xa)
            row.append((2 * S + area) // (2 * area))
        out.append(row)
    return out


def strip(pages, box, OW, table=None):
    """pages: a list of uint8 [h, w] arrays (float pages: quantise() first) -> fp32 [32, OW]"""
    table = norm() if table is None else table
    out = np.ones((OH, OW), np.float32)
    g = clip(box, [p.shape for p in pages])
    if g is None:
        return out
    p, x0, y0, cw, ch = g
    lv = levels(pages[p].tolist(), x0, y0, cw, ch)
    rows, cols = len(lv), len(lv[0])
    top, left = floordiv2(OH - rows), floordiv2(OW - cols)
    for r in range(rows):
        for c in range(cols):
            ox = left + c                                     # an oversize width: columns that fall outside are cut
            if 0 <= ox < OW:
                out[top + r, ox] = table[lv[r][c]]
    return out


def strips(pages, boxes, OW):
    return np.stack([strip(pages, b, OW) for b in boxes])[:, None] if len(boxes) else np.ones((0, 1, OH, OW), np.float32)
