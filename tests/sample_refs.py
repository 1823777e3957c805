"""Test infrastructure of the row sampler mm355_sample_rows_f32 (metamorph_amd/csrc/sample.hip): the checks and families that
tests/test_sample_gpu.py runs, the rows of tests/test_sample_edges_gpu.py, and the two CPU references that
tests/test_sample_refs_host.py holds against each other and against functional.sample_row_host.

  * round0_occupancy: an fp32 numpy mirror of the kernel up to the end of round 0 of select_key -- m, mn, fmn, scale, digit0, the bin
    each select chooses and how many values it then hands to rounds 1 .. 4.  Up to SMP_LIST = 8192 values those rounds read a list in
    LDS, above it they read the row again.  The mirror only PROVES which of the two a test row takes, and only with margin: a row meant
    for the re-read branch has n >= 1.2 * 8192, the pairs at the boundary (C - 7 = 8192 / 8193 on a finite mask, C - 5 on `points`) are
    exact by construction, so agreement with the device to the last ulp of 256 / span is never relied on.
  * hf_kept_set: what HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper keep, in fp64 with a sort, written from
    their definition; it does not call sample_row_host.
  * the families whose rows overfill one bin of round 0 (one very low finite logit stretches [fmn, m], so the bulk of the row falls into
    a few of the 256 linear bins), and `points`, rows of exact weights for the pick walk.
Pure numpy / torch on the CPU; device_draw alone touches the GPU."""
import math

import numpy as np
import torch

DEV = "cuda"
EPS = 1e-4               # the host model's band: an fp32 tree sum of a row is within ~3e-5 * Z of exact
U_MAX = 1.0 - 2.0 ** -24
#           T   top_k top_p
SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 0.9), (0.7, 50, 1.0), (1.3, 40, 0.95), (0.7, 1, 1.0)]
FAMILIES = ("peaked", "flat", "ties", "-inf entries", "all equal", "spike")
SMP_LIST = 8192          # sample.hip: the keys of round 0's bin that fit the LDS list
REREAD_MIN = math.ceil(1.2 * SMP_LIST)
CAND_CAP = 32            # the widest candidate set under which the set check still sees a wrong pick (the C = 128258 test's cap)
FMIN = float(np.finfo(np.float32).min)


def f32(v):
    return float(np.float32(v))


def family(name, R, C, g):
    x = torch.randn(R, C, generator=g)
    if name == "peaked":
        return x * 4.0
    if name == "ties":
        return torch.round(x * 4.0) / 2.0
    if name == "-inf entries":
        x[torch.rand(R, C, generator=g) < 0.3] = float("-inf")
        x[:, C // 2] = 0.25                                      # (no row of -inf alone)
    if name == "all equal":
        return torch.full((R, C), 1.25)
    if name == "spike":
        x[torch.arange(R), (torch.arange(R) * 7919 + C // 3) % C] = 80.0
    return x


def device_draw(x, T, top_k, top_p, u):
    from metamorph_amd import ops
    stats = torch.full((x.shape[0], 2), -1.0, device=DEV)
    out = ops.sample_rows(x.to(DEV).contiguous(), f32(1.0 / T), top_k, f32(top_p), u.to(DEV), stats=stats)
    assert out.dtype == torch.int32
    return out.cpu().tolist(), stats.cpu().double().numpy()


def check_row(row, T, top_k, top_p, u, out, tau, Z, who):
    """one row of the device's answer against the host model; returns the number of candidates"""
    from metamorph_amd import functional as F
    cand, lo, hi, Zh = F.sample_row_host(row, f32(1.0 / T), top_k, f32(top_p), u, eps=EPS, tau=tau)
    assert bool((row == tau).any()), (who, "tau is no value of the row", tau)
    assert lo <= tau <= hi, (who, "tau out of the band", tau, lo, hi)
    assert abs(Z - Zh) <= 1e-4 * Zh, (who, "Z", Z, Zh)
    assert out in cand, (who, "pick", out, cand, u)
    return len(cand)


# ------------------------------------------------------------------------------------------------ the kernel up to the end of round 0

def wscale_bits(C):
    """the fixed-point scale of the mass select's weights (mm355_sample_rows_f32: w * 2^bits, a row's sum below 2^62)"""
    bits = 40
    while C > (1 << (62 - bits)):
        bits -= 1
    return bits


def digit0(x, m, scale):
    """sample.hip's digit0 on an fp32 array: 255 - min((m - x) * scale, 255) truncated, -inf -> 0 (and a NaN from inf * 0 -> 0)"""
    with np.errstate(all="ignore"):
        t = (np.float32(m) - x) * np.float32(scale)
        d = 255 - np.where(t < np.float32(255.0), t, np.float32(255.0)).astype(np.int64)
    d[x == -np.inf] = 0
    return d


def _top_bin(hist, need):
    """find_bin: the highest bin b whose bins b .. 255 together reach `need` (Python ints)"""
    acc = 0
    for b in range(255, -1, -1):
        acc += int(hist[b])
        if acc >= need:
            return b
    return 0


def round0_occupancy(row, inv_t, top_k, top_p):
    """[(kind, bin, n)] for the selects the kernel runs on `row`, in their order: kind "count" (top-k) or "mass" (top-p), the bin round 0
    chooses, and the number n of row values with that digit (and x >= the top-k tau in a mass select that follows a count select) --
    what s_n holds when rounds 1 .. 4 choose between the list (n <= SMP_LIST) and the row.  Empty where no select runs: no filter, all
    values equal, or a maximum that is NaN or infinite."""
    x = np.ascontiguousarray(np.asarray(row, dtype=np.float32))
    C = x.shape[0]
    if np.isnan(x).any() or not np.isfinite(x.max()):
        return []
    m, mn = x.max(), x.min()
    fmn = x[x > -np.inf].min()
    top_k, top_p = int(top_k), np.float32(top_p)
    use_k, use_p = 0 < top_k < C, top_p < np.float32(1.0)
    if not (use_k or use_p) or not mn < m:
        return []
    with np.errstate(all="ignore"):
        span = np.float32(m - fmn)
        sc = np.float32(256.0) / span
    scale = sc if (span > 0 and sc < np.inf) else np.float32(0.0)
    d = digit0(x, m, scale)
    res = []
    keep = np.ones(C, dtype=bool)
    if use_k:
        hist = np.bincount(d, minlength=256)
        b = _top_bin(hist, top_k)
        res.append(("count", b, int(hist[b])))
        keep = x >= np.partition(x, C - top_k)[C - top_k]        # (the exact top_k-th largest value: what rounds 1 .. 4 must find)
    if use_p:
        with np.errstate(all="ignore"):
            w = np.exp((x.astype(np.float64) - float(m)) * float(np.float32(inv_t)))
        fixed = np.floor(w * 2.0 ** wscale_bits(C)).astype(np.uint64)
        hist = np.zeros(256, dtype=np.uint64)
        np.add.at(hist, d[keep], fixed[keep])
        total = sum(int(h) for h in hist)
        need = min(max(int(float(top_p) * float(total)), 1), total)
        b = _top_bin(hist, need)
        res.append(("mass", b, int((keep & (d == b)).sum())))
    return res


# ------------------------------------------------------------------------------------------------ HF's warpers, by a sort in fp64

def hf_kept_set(row, inv_t, top_k, top_p):
    """The boolean mask of the entries HF's warpers leave finite on `row`, in fp64: scores = row * inv_t; TopKLogitsWarper removes
    scores < the min(top_k, C)-th largest (top_k 0: off); TopPLogitsWarper (top_p < 1) sorts ascending, takes the softmax, removes where
    the cumulative probability is <= 1 - top_p and keeps at least the largest.  An entry that is -inf to begin with is not kept."""
    s = np.asarray(row, dtype=np.float64) * float(inv_t)
    C = s.shape[0]
    kept = s > -np.inf
    if int(top_k) > 0:
        kth = np.sort(s)[C - min(int(top_k), C)]
        kept &= ~(s < kth)
    if float(top_p) < 1.0:
        s = np.where(kept, s, -np.inf)
        order = np.argsort(s, kind="stable")                     # ascending
        with np.errstate(all="ignore"):
            e = np.exp(s[order] - s.max())
        cum = np.cumsum(e / e.sum())
        remove = cum <= 1.0 - float(top_p)
        remove[-1] = False
        kept[order[remove]] = False
    return kept


# ------------------------------------------------------------------------------------------------ rows that overfill a bin of round 0

def _cols(R, C, n, g):
    """n distinct random columns per row"""
    return torch.stack([torch.randperm(C, generator=g)[:n] for _ in range(R)])


def finite_mask(value):
    """randn * 2 with 7 columns at `value` (-1e9, finfo(float32).min: a mask written as a finite number).  (m - x) * 256 / span is
    below 1e-5 for every unmasked x, so all of them have digit 255: n = C - 7 exactly."""
    def make(R, C, g):
        x = torch.randn(R, C, generator=g) * 2.0
        x.scatter_(1, _cols(R, C, 7, g), float(value))
        return x
    return make


def low_outlier(R, C, g):
    x = torch.randn(R, C, generator=g)
    x.scatter_(1, _cols(R, C, 1, g), -80.0)
    return x


PLATEAU, PLATEAU_N, PLATEAU_TOP = 2.0, 12000, 30


def plateau(R, C, g):
    """randn - 4, PLATEAU_N columns at 2.0 and 30 distinct values in (2, 5) above them: ranks 31 .. 12030 are one value"""
    x = torch.randn(R, C, generator=g) - 4.0
    cols = _cols(R, C, PLATEAU_N + PLATEAU_TOP, g)
    x.scatter_(1, cols[:, :PLATEAU_N], PLATEAU)
    above = PLATEAU + 3.0 * torch.arange(1, PLATEAU_TOP + 1, dtype=torch.float32) / (PLATEAU_TOP + 1)
    x.scatter_(1, cols[:, PLATEAU_N:], above.expand(R, -1).contiguous())
    return x


def allowed_set(R, C, g):
    x = torch.full((R, C), float("-inf"))
    x.scatter_(1, _cols(R, C, 10, g), torch.randn(R, 10, generator=g) * 2.0)
    return x


def points(cols):
    """-inf except 0.0 at `cols`: every weight is 1.0 at any temperature, every partial sum an integer, exact in fp32"""
    def make(R, C, g=None):
        x = torch.full((R, C), float("-inf"))
        x[:, list(cols)] = 0.0
        return x
    return make


OVERFULL_FAMILIES = {"finite_mask(-1e9)": finite_mask(-1e9), "finite_mask(fmin)": finite_mask(FMIN), "low_outlier": low_outlier,
                     "plateau": plateau, "allowed_set": allowed_set}
#                 family               C       R  seed   (C = 8200 with seed 8199: the C = 8199 rows and one more column)
# seed = C, but for the finite mask at 128258: exp(2 z) weights are heavy-tailed, and with no filter the +-1e-4 Z window of seeds
# 128258 .. 128260 falls between large weights and holds 35 .. 43 light columns, above CAND_CAP; seed 128261 has at most 22
OVERFULL_CASES = [("finite_mask(-1e9)", 8199, 2, 8199),
                  ("finite_mask(-1e9)", 8200, 2, 8199),
                  ("finite_mask(-1e9)", 128258, 1, 128261),
                  ("finite_mask(fmin)", 8200, 2, 8200),
                  ("low_outlier", 128258, 1, 128258),
                  ("plateau", 20011, 2, 20011),
                  ("allowed_set", 20011, 2, 20011)]
TIE_FREE = ("finite_mask(-1e9)", "finite_mask(fmin)", "low_outlier", "allowed_set")
REREAD, LIST = "re-read", "list"
# Which branch rounds 1 .. 4 take per (family, C) and setting, one entry per select that runs (SETTINGS[0] runs none): a finite mask
# sends every select to bin 255, with C - 7 values, or with the 40 that top-k kept in a mass select after it; the outlier at -80 makes
# the bins 0.33 wide, which hold tens of values at the rank of top_k = 50 but an eighth of the row around the top_p = 0.9 threshold;
# the plateau holds the k-th value and the top-p threshold (top_k = 1 ends above it); top_k above the ten allowed values ends in the
# bin of the -inf entries, a mass select in the bin of one allowed value.  tests/test_sample_refs_host.py holds the mirror to this.
_MASK_LIST = {SETTINGS[1]: [LIST], SETTINGS[2]: [LIST], SETTINGS[3]: [LIST, LIST], SETTINGS[4]: [LIST]}
_MASK_REREAD = {SETTINGS[1]: [REREAD], SETTINGS[2]: [REREAD], SETTINGS[3]: [REREAD, LIST], SETTINGS[4]: [REREAD]}
BRANCHES = {("finite_mask(-1e9)", 8199): _MASK_LIST,           # n = 8192: the list exactly full
            ("finite_mask(-1e9)", 8200): None,                 # n = 8193: exact by construction, so held to the value, not the margin
            ("finite_mask(-1e9)", 128258): _MASK_REREAD,
            ("finite_mask(fmin)", 8200): None,                 # n = 8193 likewise
            ("low_outlier", 128258): {SETTINGS[1]: [REREAD], SETTINGS[2]: [LIST], SETTINGS[3]: [LIST, LIST], SETTINGS[4]: [LIST]},
            ("plateau", 20011): {SETTINGS[1]: [REREAD], SETTINGS[2]: [REREAD], SETTINGS[3]: [REREAD, REREAD], SETTINGS[4]: [LIST]},
            ("allowed_set", 20011): {SETTINGS[1]: [LIST], SETTINGS[2]: [REREAD], SETTINGS[3]: [REREAD, LIST], SETTINGS[4]: [LIST]}}


# A mass select that reads the row again AND has values of its bin to refuse: on the plateau every value of the bin is kept by top-k,
# so `k >= key_lo` in the re-read loop decides nothing there.  With top_k = 12000 on a finite mask, bin 255 holds the 12000 values
# that top-k kept and 8004 that it did not; T = 4 keeps the weights within a factor of ~10, so the candidate sets stay small.
KEYLO_CASE = ("finite_mask(-1e9)", 20011, 2, 20011)
KEYLO_SETTING = (4.0, 12000, 0.9)


def keylo_case():
    name, C, R, seed = KEYLO_CASE
    g = torch.Generator().manual_seed(seed)
    return OVERFULL_FAMILIES[name](R, C, g), [KEYLO_SETTING + (drawn_u(R, g),)]


def drawn_u(R, g):
    return torch.randint(0, 2 ** 24, (R,), generator=g).float() * 2.0 ** -24


def u_kinds(R, u_drawn):
    return (("drawn", u_drawn), ("0", torch.zeros(R)), ("max", torch.full((R,), U_MAX)))


def overfull_case(name, C, R, seed):
    """(x fp32 [R, C], [(T, top_k, top_p, u_drawn)] over SETTINGS) of one line of OVERFULL_CASES, the same on every call"""
    g = torch.Generator().manual_seed(seed)
    if (name, C, seed) == ("finite_mask(-1e9)", 8200, 8199):
        x = torch.cat((OVERFULL_FAMILIES[name](R, 8199, g), torch.randn(R, 1, generator=g) * 2.0), dim=1)
    else:
        x = OVERFULL_FAMILIES[name](R, C, g)
    return x, [(T, k, p, drawn_u(R, g)) for T, k, p in SETTINGS]


# ------------------------------------------------------------------------------------------------ the pick walk on exact rows

POINT_CS = (37, 1000, 8200, 128258)
SMP_NW, SMP_NCH = 16, 16


def walk_geometry(C):
    """(span_w, chunk) of stages 3 and 4: wave w owns [w * span_w, (w + 1) * span_w) in 16 chunks of a multiple of 64 columns"""
    align = 64 * SMP_NCH
    span_w = ((C + SMP_NW - 1) // SMP_NW + align - 1) // align * align
    return span_w, span_w // SMP_NCH


def walk_edges(C):
    """the columns below C at which the pick walk changes wave span, chunk or 64-column scan, and the ragged end of the row"""
    span_w, chunk = walk_geometry(C)
    e = {0, 63, 64, 511, 512, chunk - 1, chunk, span_w - 1, span_w, 15 * span_w, 15 * span_w + 15 * chunk, C - 65, C - 64, C - 1}
    return sorted(c for c in e if 0 <= c < C)


def point_sets(C):
    """at least three sorted sets of five columns that together hold every column of walk_edges(C), dealt round-robin so that
    neighbouring edges fall into different sets, filled up with random other columns"""
    edges = walk_edges(C)
    n = max(3, -(-len(edges) // 5))
    g = torch.Generator().manual_seed(C)
    rest = [c for c in torch.randperm(C, generator=g).tolist() if c not in set(edges)]
    sets = []
    for s in range(n):
        cols = edges[s::n]
        while len(cols) < 5:
            cols.append(rest.pop())
        sets.append(sorted(cols))
    return sets


POINT_US = [f32((j + 0.5) / 5) for j in range(5)] + [f32(0.2)]
POINT_FILTERS = [(1.0, 0, 1.0), (1.0, 8, 1.0)]                   # top_k = 8 > the 5 finite entries: tau = -inf through the count select


# ------------------------------------------------------------------------------------------------ extreme temperatures

TEMP_SETTINGS = [(0.05, 0, 0.9), (0.05, 50, 0.95), (20.0, 0, 0.9), (20.0, 40, 0.95)]
TEMP_FAMILIES = ("peaked", "flat", "-inf entries")
TEMP_CS = (1000, 128258)
TEMP_R = 2


def temperature_case(name, C):
    """(x fp32 [2, C] of one of the existing families, [(T, top_k, top_p, u_drawn)] over TEMP_SETTINGS), the same on every call"""
    g = torch.Generator().manual_seed(1000 * C + TEMP_FAMILIES.index(name))
    x = family(name, TEMP_R, C, g)
    return x, [(T, k, p, drawn_u(TEMP_R, g)) for T, k, p in TEMP_SETTINGS]
