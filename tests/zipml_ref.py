"""numpy restatement of ZipMLQuantizer.quantize (ml/gradient/ZipGradient.scala:70-129) with
Sort.selectKthLargest (sketch/util/Sort.java:43-58), vectorised per round, quirks included:

- the threshold is the thrNum-th largest of the h errors *and* the splitNum - h zeros behind them
  (the reference selects over its whole zero-initialised array);
- every tie with the threshold is kept;
- an odd splitNum's last singleton is dropped (the reference writes it, then overwrites the count);
- binNum = the final splitNum (B or B - 1), splits[i] = sorted[splitIndex[i + 1]] without dedup.

Where the reference throws (thrNum 0: selectKthLargest of an empty queue) or spins forever (a round
that keeps every split), `status` says so instead.  `sorted`, `r` and `t` may come from elsewhere, so
the split search can be run on the device's own prefix sums.
"""
from dataclasses import dataclass, field

import numpy as np

OK, NO_PROGRESS, THR_ZERO = "ok", "no progress", "thrNum 0"


def total_order_key(x: np.ndarray) -> np.ndarray:
    """Arrays.sort(double[])'s order as uint64: all bits of a negative flipped, the sign bit of a
    non-negative flipped (-0.0 before +0.0)."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def java_sort(x: np.ndarray) -> np.ndarray:
    """Arrays.sort of the doubles: np.sort on the total-order keys (np.sort on the floats themselves
    leaves the order of -0.0 and +0.0 open)."""
    k = np.sort(total_order_key(x))
    u = np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k)
    return u.view(np.float64)


def select_kth_largest(a: np.ndarray, k: int) -> float:
    """Sort.selectKthLargest(array, k) for 1 <= k <= len(array)."""
    assert 1 <= k <= len(a)
    i = len(a) - k
    return float(np.partition(a, i)[i])


def find_zero_idx(splits: np.ndarray, mn: float, mx: float, bin_num: int) -> int:
    """Quantizer.findZeroIdx (base/Quantizer.java:74-85)."""
    if mn > 0.0:
        return 0
    if mx < 0.0:
        return bin_num - 1
    t = 0
    while t < bin_num - 1 and splits[t] < 0.0:
        t += 1
    return t


@dataclass
class ZipResult:
    status: str
    bin_num: int = 0
    splits: np.ndarray = field(default_factory=lambda: np.zeros(0))
    min: float = 0.0
    max: float = 0.0
    zero_idx: int = 0
    rounds: int = 0
    split_index: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))
    stuck_at: int = 0  # splitNum of the round that failed

    def values(self) -> np.ndarray:
        """Quantizer.getValues (base/Quantizer.java:39-47)."""
        s, ns = self.splits, self.bin_num - 1
        v = np.empty(self.bin_num)
        v[0] = 0.5 * (self.min + s[0])
        v[1:ns] = 0.5 * (s[:ns - 1] + s[1:ns])
        v[ns] = 0.5 * (s[ns - 1] + self.max)
        return v

    def bins(self, x) -> np.ndarray:
        """indexOf of every value: the number of splits <= x (the split table ascends)."""
        return np.searchsorted(self.splits, np.asarray(x, dtype=np.float64), side="right").astype(np.int32)


def mostly_zeros(n: int = 4097, seed: int = 1) -> np.ndarray:
    """N(0,1) with exact zeros wherever a seeded uniform draw is < 0.9.  With the defaults the search
    stalls at splitNum 260 for 256 bins (most seeds get through; 1 and 4 of the first eight do not)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    x[rng.random(n) < 0.9] = 0.0
    return x


def bf16_rounded(x: np.ndarray) -> np.ndarray:
    """The finite fp32 values rounded to bfloat16 (to nearest even) and widened back: a gradient that
    went through a 16-bit format, with its many equal values and 8-bit significands."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def prefix_sums(sorted_values: np.ndarray):
    """The reference's sequential loops (ZipGradient.scala:76-83)."""
    s = np.asarray(sorted_values, dtype=np.float64)
    return np.cumsum(s), np.cumsum(s * s)


def round_errors(split_index, split_num, n, r, t):
    """errors(i) for i < splitNum / 2 (ZipGradient.scala:89-96), this association, in double."""
    h = split_num // 2
    L = split_index[0:2 * h:2]
    nxt = split_index[2:split_num:2]
    R = (np.concatenate([nxt, [n]]) if len(nxt) < h else nxt[:h]) - 1
    lm = np.maximum(L - 1, 0)
    l1 = r[R] - np.where(L == 0, 0.0, r[lm])
    l2 = t[R] - np.where(L == 0, 0.0, t[lm])
    cnt = (R - L + 1).astype(np.float64)
    mean = l1 / cnt
    return (l2 + (mean * mean) * cnt) - ((2.0 * mean) * l1)


def quantize(values, bin_num: int, sorted_values=None, r=None, t=None) -> ZipResult:
    x = np.asarray(values, dtype=np.float64)
    n = len(x)
    s = java_sort(x) if sorted_values is None else np.asarray(sorted_values, dtype=np.float64)
    if r is None or t is None:
        r, t = prefix_sums(s)
    split_num, idx, rounds = n, np.arange(n, dtype=np.int64), 0
    with np.errstate(all="ignore"):
        while split_num > bin_num:
            h = split_num // 2
            thr_num = bin_num // 2 - (split_num & 1)
            if thr_num == 0:
                return ZipResult(THR_ZERO, rounds=rounds, stuck_at=split_num)
            err = round_errors(idx, split_num, n, r, t)
            full = np.zeros(split_num)
            full[:h] = err
            thr = select_kth_largest(full, thr_num)
            keep = err >= thr
            kept = int(keep.sum())
            new_num = h + kept  # the odd singleton is not counted
            if new_num >= split_num:
                return ZipResult(NO_PROGRESS, rounds=rounds, stuck_at=split_num)
            pos = np.arange(h) + (np.cumsum(keep) - keep)
            new = np.empty(new_num, dtype=np.int64)
            new[pos] = idx[0:2 * h:2]
            new[pos[keep] + 1] = idx[1:2 * h:2][keep]
            idx, split_num, rounds = new, new_num, rounds + 1
    splits = s[idx[1:split_num]].copy()
    mn, mx = float(s[0]), float(s[n - 1])
    return ZipResult(OK, split_num, splits, mn, mx, find_zero_idx(splits, mn, mx, split_num), rounds, idx[:split_num])
