"""The sampler and the selector of the uint8 staging step (csrc/stage.hip: sample_kernel, range_kernel<NQ, true>,
sid_stage_order_stats_ws) restated in plain NumPy / Python integers, for tests/test_stage_spec_host.py (premises, CPU) and
tests/test_gpu_stage_paths.py (the kernels against it, bit for bit).  The library builds with -ffp-contract=off, so every
floating-point step of the sampler is one IEEE double operation and a Python float reproduces it.  No tests in here.

  f2key / key2f        the monotone key of a float32 and its inverse
  sample_positions     the 8192 hashed positions of the sample in the LOGICAL image (the row stride does not enter)
  brackets             per hinted fraction: the key range (lo, span, shift) the sampler forms from the sample
  begin_hint           what sid_stage_begin_hint keeps: m_valid, n_valid and per range lo, span, shift, below, inside
  select               the route of every rank of one sid_stage_order_stats_ws call, the resolving passes and their states
  order_stats          the values: np.sort of the non-NaN pixels
"""
import functools
import math

import numpy as np

K_SAMPLE = 8192              # kSample
K_HINT_BINS = 2048           # kHintBins: bins inside a hinted range; also the keys one resolving state covers
K_MAX_STATES = 8             # kMaxStates: states of one resolving pass; ranks of one radix sweep
K_MAX_HINT = 4               # kMaxHint
M_MIN = 256                  # fewer non-NaN samples than this: no range is formed
MAX_SHIFT = 14               # a rank in a range with a larger shift (a bin of more than 8 x 2048 keys) takes the radix route
NO_KEY = 0xffffffff          # the key of no non-NaN float32
OPEN_HI = 0xfffffffe
M32 = 0xffffffff


def f2key(x):
    """uint32 keys with a < b <=> key(a) < key(b) for non-NaN float32 (-0.0 directly below +0.0)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return b.view(np.float32)


@functools.lru_cache(maxsize=None)
def sample_positions(npix):
    """Flat positions (row-major, logical image) of the samples, in sample order; positions >= npix are skipped."""
    step = npix // K_SAMPLE
    out = []
    for i in range(K_SAMPLE):
        h = (i * 2654435761) & M32
        h ^= h >> 15
        h = (h * 2246822519) & M32
        h ^= h >> 13
        p = i * step + h % step if step > 0 else i
        if p < npix:
            out.append(p)
    out = np.array(out, dtype=np.int64)
    out.setflags(write=False)
    return out


def sample_keys(img):
    """Sorted keys of the non-NaN samples of a 2-D float32 image."""
    flat = np.ascontiguousarray(img, dtype=np.float32).ravel()
    v = flat[sample_positions(flat.size)]
    return np.sort(f2key(v[~np.isnan(v)]))


def bracket_ranks(f0, m):
    """(a_lo, a_hi, margin) of one fraction on m valid samples: the sample ranks floor(idx - dev) and ceil(idx + dev), and how
    far idx -+ dev is from the nearest integer (inf where the square root's argument is 0: sqrt(0) is exact on any device)."""
    f = 0.0 if f0 < 0.0 else (1.0 if f0 > 1.0 else float(f0))
    idx = f * float(m - 1)
    var = f * (1.0 - f) * float(m)
    dev = 6.0 * math.sqrt(var) + 3.0
    lo, hi = idx - dev, idx + dev
    margin = math.inf if var == 0.0 else min(abs(lo - round(lo)), abs(hi - round(hi)))
    return int(math.floor(lo)), int(math.ceil(hi)), margin


def brackets(skeys, fractions):
    """Per fraction (lo, span, shift) from the sorted valid sample keys; the state that matches nothing when m < 256."""
    m = len(skeys)
    out = []
    for f0 in fractions:
        if m < M_MIN:
            out.append((NO_KEY, 0, 0))
            continue
        a_lo, a_hi, _ = bracket_ranks(f0, m)
        klo = 0 if (a_lo < 0 or a_lo >= m) else int(skeys[a_lo])
        khi = OPEN_HI if (a_hi < 0 or a_hi >= m) else int(skeys[a_hi])
        shift = 0
        while (khi >> shift) - (klo >> shift) >= K_HINT_BINS:
            shift += 1
        lo = (klo >> shift) << shift
        out.append((lo, khi - lo, shift))
    return out


def valid_keys(img):
    flat = np.ascontiguousarray(img, dtype=np.float32).ravel()
    return np.sort(f2key(flat[~np.isnan(flat)]))


def order_stats(img, ranks):
    flat = np.ascontiguousarray(img, dtype=np.float32).ravel()
    return np.sort(flat[~np.isnan(flat)])[np.asarray(ranks, dtype=np.int64)]


def begin_hint(img, fractions):
    """What sid_stage_begin_hint keeps (the fields of sid_stage_route's first group), plus 'keys': the sorted valid keys."""
    assert 1 <= len(fractions) <= K_MAX_HINT
    skeys = sample_keys(img)
    keys = valid_keys(img).astype(np.int64)
    br = brackets(skeys, fractions)
    below = [int(np.searchsorted(keys, lo, 'left')) for lo, _, _ in br]
    inside = [int(np.searchsorted(keys, lo + span, 'right')) - b for (lo, span, _), b in zip(br, below)]
    return dict(n_hint=len(fractions), m_valid=len(skeys), n_valid=len(keys), lo=[b[0] for b in br], span=[b[1] for b in br],
                shift=[b[2] for b in br], below=below, inside=inside, keys=keys)


def plain_begin(img):
    keys = valid_keys(img).astype(np.int64)
    return dict(n_hint=0, m_valid=0, n_valid=len(keys), lo=[], span=[], shift=[], below=[], inside=[], keys=keys)


def rank_route(B, rank):
    """('direct' | 'resolved' | 'radix', range, base key of the rank's bin, states the bin needs) of one rank."""
    for q in range(B['n_hint']):
        if B['below'][q] <= rank < B['below'][q] + B['inside'][q] and B['shift'][q] <= MAX_SHIFT:
            sh = B['shift'][q]
            if sh == 0:
                return 'direct', q, int(B['keys'][rank]), 0
            base = B['lo'][q] + (((int(B['keys'][rank]) - B['lo'][q]) >> sh) << sh)
            return 'resolved', q, base, max(1, (1 << sh) >> 11)
    return 'radix', -1, 0, 0


def select(B, ranks, first_digit_known=False):
    """One sid_stage_order_stats_ws call after the begin B: counts of the three routes, the resolving passes (ranks in call
    order; a bin already in the pass shares its states; a bin that does not fit into the 8 states opens the next pass) and the
    passes over the image this call adds (`first_digit_known`: an earlier call of the same begin already took the radix route)."""
    routes = [rank_route(B, int(r)) for r in ranks]
    n_direct = sum(r[0] == 'direct' for r in routes)
    n_radix = sum(r[0] == 'radix' for r in routes)
    wants = [r for r in routes if r[0] == 'resolved']
    passes, states, w0 = 0, 0, 0
    while w0 < len(wants):
        bases, ns, w1 = [], 0, w0
        while w1 < len(wants):
            _, q, base, pieces = wants[w1]
            if (base, B['shift'][q]) not in bases:             # the same bin: the same first key and the same width
                if ns + pieces > K_MAX_STATES:
                    break
                bases.append((base, B['shift'][q]))
                ns += pieces
            w1 += 1
        passes, states, w0 = passes + 1, states + ns, w1
    image = passes
    if n_radix:
        plain = B['n_hint'] == 0
        image += (0 if (plain or first_digit_known) else 1) + 2 * ((n_radix + K_MAX_STATES - 1) // K_MAX_STATES)
    return dict(n_direct=n_direct, n_resolved=len(wants), n_radix=n_radix, resolve_passes=passes, resolve_states=states,
                image_passes_added=image, routes=[(r[0], r[3]) for r in routes])


def fraction_ranks(n, fractions):
    """The two neighbouring ranks of every (clamped) fraction of n valid pixels, ascending and distinct."""
    out = set()
    for f in fractions:
        f = min(1.0, max(0.0, float(f)))
        for d in (0, 1):
            out.add(min(n - 1, max(0, int(f * (n - 1)) + d)))
    return sorted(out)
