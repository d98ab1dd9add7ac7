"""An independent scalar restatement of the quad warp (tatt_amd/quads.py): Python ints, one pixel at a time, the matrices from a plain
`Fraction` Gaussian elimination of the eight corner equations.  Nothing here is imported from the product."""
import math
from fractions import Fraction

SHIFT = 36


def isqrt_half_up(n):
    """sqrt(n) rounded half up: the smallest r with (2 r + 1)^2 > 4 n"""
    r = 0
    while (2 * r + 1) ** 2 <= 4 * n:
        r += 1
    return r


def size(quad):
    d2 = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    p0, p1, p2, p3 = quad
    return isqrt_half_up(max(d2(p1, p0), d2(p2, p3))), isqrt_half_up(max(d2(p3, p0), d2(p2, p1)))


def solve(a, b):
    """Gaussian elimination with Fractions: a (n x n), b (n) -> x"""
    n = len(b)
    a = [[Fraction(v) for v in row] + [Fraction(r)] for row, r in zip(a, b)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                a[r] = [v - a[r][c] * w for v, w in zip(a[r], a[c])]
    return [a[r][n] for r in range(n)]


def homography(src_pts, dst_pts):
    """the 3 x 3 Fraction matrix (h22 = 1) that sends src_pts[k] to dst_pts[k], from the eight equations
    h00 u + h01 v + h02 - x (h20 u + h21 v) = x,  h10 u + h11 v + h12 - y (h20 u + h21 v) = y"""
    rows, rhs = [], []
    for (u, v), (x, y) in zip(src_pts, dst_pts):
        rows.append([u, v, 1, 0, 0, 0, -x * u, -x * v])
        rhs.append(x)
        rows.append([0, 0, 0, u, v, 1, -y * u, -y * v])
        rhs.append(y)
    h = solve(rows, rhs)
    return [h[0:3], h[3:6], [h[6], h[7], Fraction(1)]]


def apply(h, u, v):
    w = h[2][0] * u + h[2][1] * v + h[2][2]
    return (h[0][0] * u + h[0][1] * v + h[0][2]) / w, (h[1][0] * u + h[1][1] * v + h[1][2]) / w


def to_int(q, jc, ic):
    wc = q[2][0] * jc + q[2][1] * ic + q[2][2]
    return tuple(math.floor(v * 2 ** SHIFT / wc + Fraction(1, 2)) for row in q for v in row)


def matrices(quad, scale):
    """-> (m_rectify, m_paste, bbox) as the issue states them, every step spelled out on points instead of matrix products: the rational
    map in (J, I) is fitted through four points of the destination, which a projective map is determined by"""
    bw, bh = size(quad)
    rect = [(0, 0), (bw, 0), (bw, bh), (0, bh)]
    xs, ys = [p[0] for p in quad], [p[1] for p in quad]
    bx0, by0, bx1, by1 = min(xs), min(ys), max(xs), max(ys)
    # rectify: (J, I) = twice the crop coordinate -> the scene coordinate
    q_r = homography([(2 * u, 2 * v) for u, v in rect], quad)
    m_r = to_int(q_r, bw, bh)
    # paste: (J, I) = twice the coordinate inside the bounding box of the canvas -> the coordinate in the (scale bw, scale bh) line
    s = scale
    q_p = homography([(2 * s * (x - bx0), 2 * s * (y - by0)) for x, y in quad], [(s * u, s * v) for u, v in rect])
    m_p = to_int(q_p, 2 * s * (Fraction(sum(xs), 4) - bx0), 2 * s * (Fraction(sum(ys), 4) - by0))
    return m_r, m_p, (bx0, by0, bx1, by1)


def warp(src, m, out_h, out_w, dst=None, feather=0):
    """src: nested lists / array [y][x][c]; dst None: mode 0 -> nested lists; else mode 1 into a copy of dst"""
    hs, ws = len(src), len(src[0])
    out = [[[0, 0, 0] for _ in range(out_w)] for _ in range(out_h)] if dst is None else [[list(map(int, px)) for px in row] for row in dst]
    clamp = lambda v, hi: 0 if v < 0 else hi if v > hi else v
    for i in range(out_h):
        for j in range(out_w):
            J, I = 2 * j + 1, 2 * i + 1
            X, Y, Wd = (m[3 * r] * J + m[3 * r + 1] * I + m[3 * r + 2] for r in range(3))
            if Wd <= 0:
                continue
            gx, gy = (256 * X) // Wd, (256 * Y) // Wd
            if dst is not None and not (0 <= gx < 256 * ws and 0 <= gy < 256 * hs):
                continue
            fx, fy = gx - 128, gy - 128
            x0, y0, ax, ay = fx >> 8, fy >> 8, fx & 255, fy & 255
            xa, xb, ya, yb = clamp(x0, ws - 1), clamp(x0 + 1, ws - 1), clamp(y0, hs - 1), clamp(y0 + 1, hs - 1)
            for c in range(3):
                top = (256 - ax) * int(src[ya][xa][c]) + ax * int(src[ya][xb][c])
                bot = (256 - ax) * int(src[yb][xa][c]) + ax * int(src[yb][xb][c])
                v = ((256 - ay) * top + ay * bot + 32768) >> 16
                if dst is not None and feather:
                    xi, yi, D = gx >> 8, gy >> 8, feather + 1
                    a = min(min(xi, ws - 1 - xi, yi, hs - 1 - yi) + 1, D)
                    v = (2 * (a * v + (D - a) * out[i][j][c]) + D) // (2 * D)
                out[i][j][c] = v
    return out
