"""Inputs that sit on the decisions of rt_accumulate, rt_denoise_guided and rt_denoise (include/rt.h), and what the
contract says of them, derived by hand.  tests/test_filter_edges_ref.py holds the existing restatements
(accumulate_ref, guided_ref, denoise_ref) to these expectations without a GPU; tests/test_gpu_filter_edges.py holds
the kernels to the restatements and to the expectations.  profiles/filter_edges/README.md has every figure.

A  the reprojection lattice: hand-made rows (centre 0, rx, ry, rw the unit axes), so a record with point (a, b, 1)
   has (fx, fy) = (a, b) exactly; 13 values per axis that sit on the window's ends, on floorf's steps and on weights of
   exactly 0, all 169 pairs of them, seven records that decide on the denominator r2, and five plain records around
   previous texel (4, 2).  hand() derives window, taps, weights and D > 0 in plain Python, pixel by pixel.
B  steady(): guided_ref.synth with 8 samples and length 8.0 everywhere except hand-placed pixels, some of which ask
   for the spatial variance estimate (length < 4) and some of which, a float32 step away, must not.
C  one non-finite colour: where it is put, and the box of pixels it must reach.
"""
import math

import numpy as np

import accumulate_ref as A
import denoise_ref as D
import guided_ref as G

F32 = np.float32
INF = float("inf")
NAN = float("nan")
MISS = 0xFFFFFFFF


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- A: the reprojection lattice -------------------------------------------------------------------------------------

LW, LH = 24, 8                                            # no multiple of 16 or 64 across, less than a block row down
KW_A = dict(max_history=16.0, normal_cos=0.98, plane_tolerance=INF)
ROWS = {"centre": np.zeros(3, F32), "rx": np.array([1, 0, 0], F32), "ry": np.array([0, 1, 0], F32),
        "rw": np.array([0, 0, 1], F32)}
COLOUR = (100.0, 200.0, 300.0)                            # no blend of the history's colours (at most 24, 8, 0.5)
POISONED_TEXEL = (4, 2)                                   # the variant: previous history there is +inf in green
Z = F32(2.0 ** -130)                                      # a float32 denormal; 3 Z and 2 Z are exact


def axis_values(n):
    """The 13 values of one axis (n = W or H), float32."""
    f = F32
    return [np.nextafter(f(-1), f(-2)),                   # fails the window
            f(-1),                                        # passes; the only inside tap has weight 0: D = 0, reset
            np.nextafter(f(-1), f(0)),                    # column 0 with a weight of one ulp: kept
            f(-0.5),                                      # left tap outside
            np.nextafter(f(0), f(-1)),                    # a denormal: floorf = -1, the weight rounds to 1
            f(-0.0), f(0.0),                              # ix = 0, wx = +0
            f(0.25), f(n - 1.5),                          # interior
            f(3.0),                                       # interior integer: the right tap is valid with b = 0
            f(n - 1),                                     # right tap outside
            np.nextafter(f(n), f(0)),                     # the last value inside the window
            f(n)]                                         # fails the window


# (point, expected): None = reset, else the (fx, fy) the pixel is kept at
DENOMINATORS = (((3.0, 2.0, 0.0), None),                  # quotient infinite
                ((0.0, 0.0, 0.0), None),                  # 0 / 0
                ((-3.0, -2.0, -1.0), None),               # quotient in the window, behind the camera
                ((1.0, 0.0, 1e-30), None),                # fx = 1e30: finite and beyond int
                ((NAN, 2.0, 1.0), None),
                ((3.0, 2.0, INF), None),                  # 0 * inf in r0
                ((F32(3) * Z, F32(2) * Z, Z), (3.0, 2.0)))    # products and quotients exact: kept
# The per-axis table has no 2.0, so the lattice adds the plain (3, 2) pixel the denormal one must equal, and four more
# around previous texel (4, 2): weights all nonzero; weight 1 on it; b = 0 through wy; b = 0 through both.
PLAIN = ((3.0, 2.0), (3.5, 1.5), (4.0, 2.0), (4.0, 1.0), (3.0, 1.0))
N_PAIRS = 169
K_DENORMAL = N_PAIRS + len(DENOMINATORS) - 1
K_PLAIN = N_PAIRS + len(DENOMINATORS)                     # the plain (3, 2) pixel


def lattice_points():
    """Per pixel k of the LW x LH image, row-major: (point | None for a miss, expected (fx, fy) | None)."""
    xs, ys = axis_values(LW), axis_values(LH)
    pts = [((xs[k % 13], ys[k // 13], F32(1)), (xs[k % 13], ys[k // 13])) for k in range(N_PAIRS)]
    pts += [(p, e) for p, e in DENOMINATORS]
    pts += [((F32(a), F32(b), F32(1)), (a, b)) for a, b in PLAIN]
    pts += [(None, None)] * (LW * LH - len(pts))
    return pts


def _axis(f, n, lo, hi):
    """One axis by the contract: the window, floorf, and the inside taps [(index, weight)]; None = outside the window."""
    f = float(f)
    if not (f >= -1.0 if lo == "ge" else f > -1.0) or not (f < n if hi == "lt" else f <= n):
        return None                                       # a NaN fails the first comparison
    i = math.floor(f)
    w = F32(f) - F32(i)                                   # one float32 subtraction
    return [(q, b) for q, b in ((i, F32(1) - w), (i + 1, w)) if 0 <= q < n]


def hand(lo="ge", hi="lt", skip_zero=False):
    """The contract on the lattice in plain Python, with no call into accumulate_ref: per pixel None (reset) or
    {"taps": [((qx, qy), b)] in tap order, "D", "r", "g"}: the inside taps (every inside tap is valid: all previous
    records are alike), D = sum b with each product rounded, and the bilinear value of qx + 1 and qy + 1 in float64.
    The faults of the issue: lo="gt" (fx > -1), hi="le" (fx <= W), skip_zero (a tap with b == 0 is left out)."""
    out = []
    for point, want in lattice_points():
        ax = None if want is None else _axis(want[0], LW, lo, hi)
        ay = None if want is None else _axis(want[1], LH, lo, hi)
        if ax is None or ay is None:
            out.append(None)
            continue
        taps = [((qx, qy), bx * by) for qy, by in ay for qx, bx in ax]        # (0,0), (1,0), (0,1), (1,1)
        if skip_zero:
            taps = [t for t in taps if t[1] != 0]
        Dn = F32(0)
        for _, b in taps:
            assert type(b) is F32
            Dn = Dn + b
        if not Dn > 0:
            out.append(None)
            continue
        sx, sy = sum(float(b) for _, b in ax), sum(float(b) for _, b in ay)
        out.append({"taps": taps, "D": Dn, "r": sum(float(b) * (q + 1) for q, b in ax) / sx,
                    "g": sum(float(b) * (q + 1) for q, b in ay) / sy})
    return out


def hand_reset(**fault):
    return np.array([h is None for h in hand(**fault)]).reshape(LH, LW)


def hand_reaches(texel, **fault):
    """Kept pixels that have `texel` among their taps, a tap of weight 0 included."""
    return np.array([h is not None and any(q == texel for q, _ in h["taps"]) for h in hand(**fault)]).reshape(LH, LW)


_lattice = {}


def lattice(variant=False):
    """The lattice's inputs and the restatements' results, computed once, shared and read-only.  variant: previous
    history texel POISONED_TEXEL is +inf in green."""
    if variant not in _lattice:
        n = LW * LH
        rng = np.random.default_rng(424242)
        dt = A.hit_dtype()
        hits, prev = np.zeros(n, dt), np.zeros(n, dt)
        for k, (point, _) in enumerate(lattice_points()):
            if point is None:
                hits[k]["t"], hits[k]["instance"] = F32(INF), MISS
            else:
                hits[k]["t"], hits[k]["instance"], hits[k]["point"], hits[k]["normal"] = 1.0, 0, point, (0.0, 0.0, 1.0)
        prev["t"], prev["instance"], prev["point"], prev["normal"] = 1.0, 0, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)
        qy, qx = np.mgrid[0:LH, 0:LW]
        hist = np.stack([qx + 1.0, qy + 1.0, np.full((LH, LW), 0.5), 1.0 + (qx + 3 * qy) % 19 + 0.25 * (qx % 4)],
                        axis=-1).astype(F32)
        if variant:
            hist[POISONED_TEXEL[1], POISONED_TEXEL[0], 1] = INF
        m1 = rng.uniform(0.0, 1.5, (LH, LW))
        g = {"color": np.tile(np.array(COLOUR, F32), (LH, LW, 1)), "hits": hits.reshape(LH, LW),
             "prev_hits": prev.reshape(LH, LW), "prev_history": hist, "view": ROWS,
             "prev_moments": np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.3, (LH, LW))], axis=-1).astype(F32),
             "albedo": rng.uniform(0.05, 1.0, (LH, LW, 3)).astype(F32)}
        g["albedo"].reshape(-1, 3)[K_DENORMAL] = g["albedo"].reshape(-1, 3)[K_PLAIN]     # so their moments agree too
        acc = (g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"])
        mom = (g["color"], g["albedo"], g["hits"], g["prev_hits"], g["prev_history"], g["prev_moments"], g["view"])
        with np.errstate(all="ignore"):
            g["ref32"], g["valid32"] = A.accumulate(*acc, dtype=np.float32, **KW_A)
            g["ref64"], g["valid64"] = A.accumulate(*acc, dtype=np.float64, **KW_A)
            g["moments32"] = G.accumulate_moments(*mom, dtype=np.float32, **KW_A)
        for arr in g.values():
            for a in (arr if isinstance(arr, tuple) else (arr,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _lattice[variant] = g
    return _lattice[variant]


def restatement_reaches(valid, texel):
    """Pixels whose valid taps, as the restatement returns them, include `texel`; the taps' coordinates are
    floor(fx) + tx, floor(fy) + ty of the pixel's expected (fx, fy)."""
    out = np.zeros((LH, LW), bool)
    for k, (_, want) in enumerate(lattice_points()):
        for tap in range(4):
            if valid[k // LW, k % LW, tap]:
                q = (math.floor(float(want[0])) + (tap & 1), math.floor(float(want[1])) + (tap >> 1))
                out[k // LW, k % LW] |= q == texel
    return out


# ---- B: fractional lengths and sparse requests -----------------------------------------------------------------------

BELOW_4, ABOVE_4 = float(np.nextafter(F32(4), F32(0))), float(np.nextafter(F32(4), F32(8)))
# name: (width, height, iterations, {(x, y): (samples, length)} that ask, the same that must not ask)
STEADY = {
    # 3 x 3 tiles, the last column 3 wide and the last row 2 high; tiles (2,0), (2,1), (0,2), (1,2) hold no request,
    # and every asking pixel of tiles (0,0), (1,0), (1,1) sits at a tile corner: its window reads tiles that left early
    "35x34": (35, 34, 3,
              {(0, 0): (1, 1.0), (15, 15): (3, 3.0), (16, 16): (4, BELOW_4), (31, 15): (1, 1.25), (34, 33): (2, 2.5),
               (32, 32): (3, 3.75), (3, 20): (1, 1.0)},
              {(15, 16): (4, 4.0), (16, 15): (4, ABOVE_4), (33, 33): (4, 4.0)}),
    # one asking pixel, the far corner of a partial tile; every other tile leaves at the vote
    "33x18": (33, 18, 2, {(32, 17): (2, 2.5)}, {}),
}


def placed(name):
    _, _, _, ask, quiet = STEADY[name]
    return tuple(sorted({**ask, **quiet}.items()))


def steady(width, height, pixels):
    """guided_ref.synth's guides, truth and sample noise; 8 samples and length 8.0 everywhere except `pixels`, a tuple
    of ((x, y), (samples, length)).  The moments are always those of the pixel's own samples."""
    return G.synth(width, height, lengths=tuple(pixels))


def steady_reference(name):
    W, H, it, _, _ = STEADY[name]
    return G.reference(W, H, it, lengths=placed(name))


def estimates(r):
    """(spatial, temporal) v_0 of a reference's inputs everywhere, float64."""
    g = r["g"]
    kw = dict(sigma_normal=r["kw"]["sigma_normal"], sigma_plane=r["kw"]["sigma_plane"])
    args = (g["history"], r["moments"], g["normal"], g["point"], g["miss"])
    return G.variance(*args, threshold=1e9, **kw), G.variance(*args, threshold=0, **kw)


# ---- C: one non-finite colour ----------------------------------------------------------------------------------------

POISON_CASES = ((17, 17, 1), (37, 23, 2), (65, 9, 3), (257, 5, 4))     # the last reaches the row form at steps 4 and 8
POISON_VALUES = (NAN, INF)
POISON_CHANNEL = 1


def positions(miss):
    """(x, y) of the four places: two corners, the centre, and the first sky pixel of the middle row that has a hit
    to its left."""
    H, W = miss.shape
    row = H // 2
    edge = next(x for x in range(1, W) if miss[row, x] and not miss[row, x - 1])
    return ((0, 0), (W // 2, H // 2), (W - 1, H - 1), (edge, row))


def poisoned(image, z, value):
    out = np.array(image, F32)
    out[z[1], z[0], POISON_CHANNEL] = value
    return out


def box(width, height, iterations, z):
    """The pixels within 2 (2^iterations - 1) of z in both axes: what the passes' taps reach."""
    r = 2 * ((1 << iterations) - 1)
    yy, xx = np.mgrid[0:height, 0:width]
    return (np.abs(xx - z[0]) <= r) & (np.abs(yy - z[1]) <= r)


def shielded(miss, iterations, z):
    """What a colour filter whose taps return early on miss(p) != miss(q) would spread instead: the fault
    `if (nq.w != np.w) return;` at the top of add_tap, as a set computation."""
    H, W = miss.shape
    bad = np.zeros((H, W), bool)
    bad[z[1], z[0]] = True
    for i in range(iterations):
        s, nxt = 1 << i, bad.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if not D.lands(W, H, s, dx, dy):
                    continue
                p, q = G._shifted(H, W, s * dx, s * dy)
                nxt[p] |= bad[q] & (miss[p] == miss[q])
        bad = nxt
    return bad
