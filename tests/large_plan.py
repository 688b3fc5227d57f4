"""Python twins of the large sort's host arithmetic (oclradixsort_amd/csrc/large_plan.hpp): slab and tile sizes, the two layouts'
capacities, the form a sort prefers, the three shared conditions and the fallback chain (plain Python, no GPU;
tests/test_large_plan.py checks this module against the header on the CPU, tests/test_gpu_slab_edges.py uses it on the device).

The twins restate capacities and decisions, not byte offsets: the chain's twin is given the candidates' totals.
"""
MI = 1 << 20
U32, KV32, U64, SOA32 = 0, 1, 2, 3   # ADLHIP_ELEM_*

FULL_PCT, LEAN_PCT = 50, 12   # kFullHeadroomPct, kLeanHeadroomPct (large_plan.hpp)
STRIDE0 = 1536                # kMsd2Stride0 (large_plan.hpp)
SMALL_MAX = 16384             # kSmallMax = kMsd2Min
CURSOR_MAX = {4: 1088 << 20, 8: (1 << 28) + (1 << 22)}   # kMsd2MaxU32, kMsd2MaxU64
STABLE_MAX = (1 << 28) + (1 << 22)                       # kMsd2sMax
SLAB_IN_TMP_MIN = 16 << 20                               # kSlabInTmpMin


def _align_up(x, a):
    return (x + a - 1) // a * a


def _sd(mean):
    """the host's integer standard deviation: the smallest sd >= 1 with sd * sd >= mean"""
    sd = 1
    while sd * sd < mean:
        sd += 1
    return sd


def msd2_tier_b(n, slots=65536, fine=False):
    """large_plan.hpp msd2_tier_b: the finish's tile that holds the mean segment + 7.5 sd"""
    mean = (n + slots - 1) // slots
    need = mean + (15 * _sd(mean) + 1) // 2
    if fine and 2560 < need <= 4096:
        return 3072 if need <= 3072 else 4096
    if need <= 5120:
        return 1280 if need <= 832 else STRIDE0 if need <= 1280 else 2560 if need <= 2560 else 5120
    return 8192 if need <= 8192 else 12288 if need <= 12288 else 16384 if need <= 16384 else 20480


def msd2_stride_b(n, slots=65536, fine=False, lean=False):
    """large_plan.hpp msd2_stride_b: mean + 50 % (lean: the mean), or mean + 7.5 sd where that is more, + 8, in steps of 64,
    at most the tile"""
    mean = (n + slots - 1) // slots
    want = _align_up(max(mean if lean else mean + mean // 2, mean + (15 * _sd(mean) + 1) // 2) + 8, 64)
    return min(want, msd2_tier_b(n, slots, fine))


def msd2_seg_shift(n, bin_finish):
    """large_plan.hpp msd2_seg_shift: width w of the second digit (256 << w segments)"""
    max_n = (1 << 40) if bin_finish else (16 << 20)
    if n >= max_n:
        return 8
    w = 2
    while w < 8 and (n >> (8 + w)) > 1024:
        w += 1
    return w


def msd2_layout(n, elem_bytes, headroom_pct=FULL_PCT):
    """large_plan.hpp msd2_layout (cursor form): bucket slab stride_a, segment slabs stride_b, finish tile tier_b"""
    w = msd2_seg_shift(n, elem_bytes == 8)
    fine = elem_bytes == 4 and w == 8
    return dict(stride_a=_align_up(n // 256 + (n // 256) * headroom_pct // 100 + 4096, 64), seg_shift=w,
                stride_b=msd2_stride_b(n, 256 << w, fine), tier_b=msd2_tier_b(n, 256 << w, fine))


def msd2s_layout(n, elem_bytes=8, slab16=False, lean=False):
    """large_plan.hpp msd2s_layout (stable and hybrid forms): 16 chains, each a slice of the input; one sub-slab of stride_a per
    (bucket, chain); slab16 = whole u32 keys (65536 segments, 16-bit second slab)"""
    tile = 8192 if elem_bytes == 8 else 16384   # msd2s_tile (large_plan.hpp)
    pieces = 16
    slice_ = _align_up((n + pieces - 1) // pieces, tile)
    mean = slice_ // 256
    w = 8 if slab16 else msd2_seg_shift(n, False)
    return dict(pieces=pieces, slice=slice_, stride_a=_align_up(mean + (0 if lean else mean // 2) + 8 * _sd(mean) + 64, 64),
                seg_shift=w, stride_b=msd2_stride_b(n, 256 << w, slab16, lean), tier_b=msd2_tier_b(n, 256 << w, slab16))


def large_sort_form(kind, n, sort_bits, knob, rank=1, persist=1, resident=256):
    """large_plan.hpp large_sort_form: 'cursor' / 'stable' / 'hybrid' / None for a sort of n elements of `kind` with the
    "sort.msd2" knob (8-bit digits, automatic algorithm; resident = "debug.resident_wgs", at least 256 on a whole device)"""
    if knob == 0 or sort_bits < 16 or resident < 256:
        return None
    elem_bytes = 4 if kind == U32 else 8
    max_bits = 64 if kind == U64 else 32
    keys = kind in (U32, U64)
    forced, whole = knob >= 2, sort_bits == max_bits
    if rank != 1 and (keys or n > (96 << 20) or msd2_tier_b(n, 256 << msd2_seg_shift(n, False)) > 2560):
        return None
    if not keys:
        return "stable" if (n > (16384 if forced else MI)) and n <= (1 << 28) + (1 << 22) else None
    if n <= (16384 if forced or elem_bytes == 8 else 2 * MI):
        return None
    cursor_max = (1088 << 20) if elem_bytes == 4 else (1 << 28) + (1 << 22)
    stable_max = (1 << 28) + (1 << 22)
    if not whole or knob == 3:
        return "stable" if n <= stable_max else None
    if knob == 4:
        return "cursor" if n <= cursor_max else None
    if knob == 5:
        return "hybrid" if n <= stable_max else None
    if elem_bytes == 4 and (192 << 20 if persist else 96 << 20) <= n <= stable_max:
        return "hybrid"
    if elem_bytes == 8 and (48 << 20) <= n <= stable_max:
        return "stable"
    return "cursor" if n <= cursor_max else None


# ---------------------------------------------------------------------------------------------
# the plan: the three shared conditions, the fallback chain, what follows from the chosen layout
# ---------------------------------------------------------------------------------------------
def elem_bytes_of(kind):
    return 4 if kind == U32 else 8


def is_whole(kind, sort_bits):
    return sort_bits == (64 if kind == U64 else 32)


def large_slab16(elem_bytes, whole):
    """large_plan.hpp large_slab16: whole u32 keys get the 16-bit second slab"""
    return elem_bytes == 4 and whole


def cursor_eligible(elem_bytes, keys, whole, n):
    """large_plan.hpp cursor_eligible"""
    return keys and whole and n <= CURSOR_MAX[elem_bytes]


def stable_eligible(n):
    """large_plan.hpp stable_eligible"""
    return n <= STABLE_MAX


def large_fallbacks(kind, n, sort_bits):
    """large_plan.hpp large_fallbacks: the (form, lean) a sort falls back to when its preferred form does not fit, in the order tried"""
    eb, whole = elem_bytes_of(kind), is_whole(kind, sort_bits)
    out = []
    if cursor_eligible(eb, kind in (U32, U64), whole, n):
        out += [("cursor", False), ("cursor", True)]
    if stable_eligible(n):
        out.append(("stable", True))
    return out


def choose(preferred, fallbacks, totals, offered):
    """large_plan.hpp large_plan's chain: the preferred form at full head-room if its layout fits `offered` bytes, else the first
    fallback that does, else nothing.  totals[(layout kind, lean)] = the layout's bytes, layout kind 'cursor' or 'stable' (the hybrid
    form has the stable form's layout).  Returns (form, lean, headroom per cent of the cursor form's first slabs)."""
    if preferred is None:
        return (None, False, FULL_PCT)
    for form, lean in [(preferred, False)] + list(fallbacks):
        if totals[("cursor" if form == "cursor" else "stable", lean)] <= offered:
            return (form, lean, LEAN_PCT if form == "cursor" and lean else FULL_PCT)
    return (None, False, FULL_PCT)


def layout_of(kind, n, sort_bits, form, lean):
    """the twin layout of a chosen (form, lean), as large_plan.hpp large_layout builds it"""
    eb = elem_bytes_of(kind)
    if form == "cursor":
        return msd2_layout(n, eb, LEAN_PCT if lean else FULL_PCT)
    return msd2s_layout(n, eb, large_slab16(eb, is_whole(kind, sort_bits)), lean)


def plan_slab16(kind, sort_bits, L):
    """LargePlan::slab16: the second slab holds the keys' low 16 bits"""
    return large_slab16(elem_bytes_of(kind), is_whole(kind, sort_bits)) and L["seg_shift"] == 8


def slab_b_in_tmp(kind, n, sort_bits, L):
    """LargeLayout::slab_b_in_tmp: the 16-bit second slab lies in the caller's n-element scratch array"""
    return plan_slab16(kind, sort_bits, L) and n >= SLAB_IN_TMP_MIN and (256 << L["seg_shift"]) * L["stride_b"] * 2 <= n * 4


def bin_finish(kind, n, sort_bits, L):
    """LargePlan::bin with "sort.binfinish" = 1 (large_plan.hpp use_bin_finish): whole u64 keys from 24 Mi keys, or at any n with a
    narrow second digit"""
    return kind == U64 and is_whole(kind, sort_bits) and (L["seg_shift"] < 8 or n >= (24 << 20))


def large_work_bytes_at(kind, n, sort_bits, level, totals):
    """large_plan.hpp large_work_bytes_at (levels 1 and 2) from the candidates' totals; the "sort.msd2" knob plays no part"""
    if not (n > SMALL_MAX and sort_bits >= 16):
        return 0
    fb = large_fallbacks(kind, n, sort_bits)
    if level == 2:
        lean = [c for c in fb if c[1]]
        return totals[lean[0]] if lean else 0
    full = [("stable", False)] if stable_eligible(n) else []
    full += [c for c in fb if not c[1]]
    return max([totals[c] for c in full], default=0)
