"""numpy model of the prefix-sum tree of sketchml_amd/csrc/skml_zip.hip (k_zip_scan_dd, zip_scan_level)
and the exact sums it is tested against.

The model does the kernel's additions in the kernel's order, every one of them in IEEE double as
numpy does it: zdd_add on (hi, lo) pairs; a thread's 8 values in order; the wave's Hillis-Steele scan
over the 64 thread totals; the 4 wave totals in order starting from a zero pair; output = (workgroup
offset + (wave offset + lane offset)) + the thread's own prefix; the workgroup totals through the same
tree, scanned in place as pairs; hi alone at the leaves.  The leaves' squares are taken exactly: numpy
has no fma, so p + e = s * s comes from a Veltkamp split and Dekker's product, which gives the e that
fma(s, s, -p) gives whenever neither over- nor underflows.  Entries past n are zero pairs and take
part in the additions as they do on the device.

exact_prefix_sums is the other side: cumulative sums in Python integers, each rounded to double once,
to nearest even (float(int) rounds correctly).
"""
import numpy as np

THREAD, LANES, WAVES = 8, 64, 4
BLOCK = THREAD * LANES * WAVES  # 2,048 values per workgroup


def zdd_add(xh, xl, yh, yl):
    """zdd_add of skml_zip.hip, elementwise."""
    s = xh + yh
    bb = s - xh
    e = (xh - (s - bb)) + (yh - bb)
    e = e + (xl + yl)
    hi = s + e
    return hi, e - (hi - s)


def two_square(v):
    """(p, e) with p = fl(v * v) and p + e = v * v exactly."""
    v = np.asarray(v, dtype=np.float64)
    p = v * v
    c = v * 134217729.0  # 2^27 + 1
    h = c - (c - v)
    l = v - h
    return p, ((h * h - p) + 2.0 * (h * l)) + l * l


def _scan_pairs(hi, lo, add):
    """Inclusive scan of the pairs (hi[i], lo[i]) as one level of the tree and the levels above it."""
    n = len(hi)
    nb = -(-n // BLOCK)
    ah, al = np.zeros(nb * BLOCK), np.zeros(nb * BLOCK)
    ah[:n], al[:n] = hi, lo
    ah, al = ah.reshape(nb, WAVES, LANES, THREAD), al.reshape(nb, WAVES, LANES, THREAD)
    for k in range(1, THREAD):  # the thread's own prefix
        ah[..., k], al[..., k] = add(ah[..., k - 1], al[..., k - 1], ah[..., k], al[..., k])
    th, tl = ah[..., THREAD - 1].copy(), al[..., THREAD - 1].copy()
    d = 1
    while d < LANES:  # Hillis-Steele over the lanes
        nh, nl = add(th[..., :-d], tl[..., :-d], th[..., d:], tl[..., d:])
        th[..., d:], tl[..., d:] = nh, nl
        d <<= 1
    eh, el = np.zeros_like(th), np.zeros_like(tl)  # the lanes before this one
    eh[..., 1:], el[..., 1:] = th[..., :-1], tl[..., :-1]
    wh, wl = np.zeros((nb, WAVES)), np.zeros((nb, WAVES))  # the waves before this one, in order
    for w in range(1, WAVES):
        wh[:, w], wl[:, w] = add(wh[:, w - 1], wl[:, w - 1], th[:, w - 1, LANES - 1], tl[:, w - 1, LANES - 1])
    oh, ol = add(wh[:, :, None], wl[:, :, None], eh, el)
    if nb > 1:
        toth, totl = add(wh[:, WAVES - 1], wl[:, WAVES - 1], th[:, WAVES - 1, LANES - 1], tl[:, WAVES - 1, LANES - 1])
        offh, offl = _scan_pairs(toth, totl, add)
        nh, nl = add(offh[:-1, None, None], offl[:-1, None, None], oh[1:], ol[1:])
        oh[1:], ol[1:] = nh, nl
    rh, rl = add(oh[..., None], ol[..., None], ah, al)
    return rh.reshape(-1)[:n], rl.reshape(-1)[:n]


def zdd_add_plain(xh, xl, yh, yl):
    """zdd_add with the low part lost: the tree in plain double."""
    s = xh + yh
    return s, np.zeros_like(s)


def scan(sorted_values, add=zdd_add):
    """(r, t) of the device's tree over the sorted doubles.  add = zdd_add_plain gives what a tree
    without the compensation would: the sums the tests must tell from the device's."""
    s = np.ascontiguousarray(sorted_values, dtype=np.float64)
    with np.errstate(all="ignore"):
        r, _ = _scan_pairs(s, np.zeros_like(s), add)
        t, _ = _scan_pairs(*two_square(s), add)
    return r, t


def as_ints(a, e0):
    """The doubles as Python integers in units of 2^e0 (every value a multiple of it)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = (m * float(1 << 53)).astype(np.int64).astype(object)
    sh = np.where(a == 0, 0, e.astype(np.int64) - 53 - e0)
    assert sh.min() >= 0
    return mi << sh.astype(object)


def exact_prefix_sums(sorted_values):
    """(r, t): the exact sums of the values and of their exact squares, each rounded once to double."""
    s = np.ascontiguousarray(sorted_values, dtype=np.float64)
    nz = s[s != 0]
    e0 = int(np.frexp(np.abs(nz).min())[1]) - 53 if len(nz) else 0
    si = as_ints(s, e0)
    r = np.ldexp(np.cumsum(si).astype(np.float64), e0)  # object -> float64 is float(int): to nearest even
    t = np.ldexp(np.cumsum(si * si).astype(np.float64), 2 * e0)
    return r, t
