"""Constructed descriptor sets for the Hamming matcher (include/sid_ft.h), each with its claim.

A case is a dict:
    name     its id
    d1, d2   uint8 [n1,32], [n2,32]
    env      {'SID_FT_NO_MFMA': '1'} or {}: the switches the case runs under
    plan     what sid_ft_debug_plan must report: mfma, chunk, nchunks, n1pad, n2pad (literal numbers, worked out by hand from
             csrc/ft_plan.h; plan_spec below restates the header and tests/test_ft_cases_host.py holds the two together)
    claims   [(query, slot, train index, distance)]: results known BY CONSTRUCTION (slot 0: nearest, 1: runner-up)
    asserted the queries a test compares with the oracle: all of them, or for the large cases the first and the last block
             of 256 queries plus every query with a claim (at most 1024)

Background descriptors are random: about 128 bits (never fewer than ~80) from everything else.  Planted descriptors are a
descriptor with exactly k chosen bits flipped.  Where several queries must have their nearest and their runner-up at the SAME
few train indices (chunk edges, batch edges) the train descriptors at those indices form a cluster: T_i = B with the 8 bits of
group i flipped (16 bits between any two of them), and a query is B with parts of two groups flipped -
    order (a, b):  all of group a and 4 bits of group b:  4 from T_a, 12 from T_b, 20 from the rest of the cluster
    tie   (a, b):  4 bits of group a, 4 bits of group b:  8 from T_a and from T_b, 16 from the rest: the smaller index first
"""
import functools

import numpy as np

NO_MFMA = {'SID_FT_NO_MFMA': '1'}


def plan_spec(n1, n2, no_mfma=False):
    """csrc/ft_plan.h in Python integers: the fields of sid_ft_debug_plan."""
    if n1 * n2 >= 1 << 24 and n2 >= 1024 and not no_mfma:
        n1pad, n2pad = -(-max(n1, 1) // 256) * 256, -(-max(n2, 1) // 256) * 256
        qblocks, batches = n1pad // 256, n2pad // 256
        want = min(max(1, -(-512 // qblocks)), batches)
        per = -(-batches // want)
        return dict(mfma=1, chunk=per * 256, nchunks=-(-batches // per), n1pad=n1pad, n2pad=n2pad)
    qblocks = -(-n1 // 256)
    want = max(1, -(-2048 // max(qblocks, 1)))
    c = min(max(256, -(-n2 // want)), max(n2, 1))
    return dict(mfma=0, chunk=c, nchunks=max(1, -(-n2 // c)), n1pad=n1, n2pad=n2)


def workspace_spec(n1, n2):
    """sid_ft_workspace_bytes: the larger of both forms' needs (regions start 256 bytes apart at the least)."""
    up = lambda b: -(-b // 256) * 256
    valu = 8 * max(n1, 1) * plan_spec(n1, n2, True)['nchunks']
    n1pad, n2pad = -(-max(n1, 1) // 256) * 256, -(-max(n2, 1) // 256) * 256
    qblocks, batches = n1pad // 256, n2pad // 256
    per = -(-batches // min(max(1, -(-512 // qblocks)), batches))
    return max(valu, up(8 * max(n1, 1) * -(-batches // per)) + 256 * n1pad + 256 * n2pad + up(4 * n2pad))


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(desc, bits):
    """A copy of one descriptor with the given bit positions (0..255) flipped."""
    m = np.zeros(256, dtype=np.uint8)
    m[list(bits)] = 1
    return desc ^ np.packbits(m)


def _plan(mfma, chunk, nchunks, n1pad, n2pad):
    return dict(mfma=mfma, chunk=chunk, nchunks=nchunks, n1pad=n1pad, n2pad=n2pad)


def _asserted(n1, claims):
    if n1 <= 1024:
        return np.arange(n1)
    sel = set(range(256)) | set(range(n1 - 256, n1)) | {c[0] for c in claims}
    assert len(sel) <= 1024
    return np.array(sorted(sel))


def _case(name, d1, d2, plan, claims, env=None):
    return dict(name=name, d1=d1, d2=d2, env=dict(env or {}), plan=plan, claims=list(claims), asserted=_asserted(len(d1), claims))


def _cluster(rng, n1, n2, specials, orders, ties, queries):
    """Random sets with a cluster at the train indices `specials`; query queries[k] is built for the k-th entry of
    orders + ties (pairs of positions in `specials`)."""
    d1, d2 = rand_desc(rng, n1), rand_desc(rng, n2)
    base = rand_desc(rng, 1)[0]
    group = lambda i: range(8 * i, 8 * i + 8)
    for i, j in enumerate(specials):
        d2[j] = flipped(base, group(i))
    claims = []
    todo = [(a, b, False) for a, b in orders] + [(a, b, True) for a, b in ties]
    assert len(todo) <= len(queries) and len(specials) <= 32
    for q, (a, b, tie) in zip(queries, todo):
        if tie:
            d1[q] = flipped(base, list(group(a))[:4] + list(group(b))[:4])
            lo, hi = sorted((specials[a], specials[b]))
            claims += [(q, 0, lo, 8), (q, 1, hi, 8)]
        else:
            d1[q] = flipped(base, list(group(a)) + list(group(b))[:4])
            claims += [(q, 0, specials[a], 4), (q, 1, specials[b], 12)]
    return d1, d2, claims


def _all_pairs(n):
    orders = [(a, b) for a in range(n) for b in range(n) if a != b]
    ties = [(a, b) for a in range(n) for b in range(a + 1, n)]
    return orders, ties


def _spread(n1, count):
    """`count` distinct query indices that include both ends of the first two and of the last block of 256 queries."""
    must = [q for q in (0, 255, 256, 257, 511, n1 - 257, n1 - 256, n1 - 1) if 0 <= q < n1]
    rest = [q for q in np.linspace(0, n1 - 1, 4 * count).astype(int).tolist() if q not in must]
    out = list(dict.fromkeys(must + rest))[:count]
    assert len(out) == count
    return out


def _valu_cases(rng):
    out = []
    # 1 x 2, 1 x 255, 255 x 256: one chunk; the idle lanes of the only block clamp their query; remainders 2, 3, 0 of the unroll by 4
    d1 = rand_desc(rng, 1)
    d2 = np.stack([flipped(d1[0], range(7)), flipped(d1[0], range(3))])
    out.append(_case('valu_1x2', d1, d2, _plan(0, 2, 1, 1, 2), [(0, 0, 1, 3), (0, 1, 0, 7)]))
    d1, d2 = rand_desc(rng, 1), rand_desc(rng, 255)
    d2[254], d2[252] = flipped(d1[0], range(2)), flipped(d1[0], range(100, 109))
    out.append(_case('valu_1x255', d1, d2, _plan(0, 255, 1, 1, 255), [(0, 0, 254, 2), (0, 1, 252, 9)]))
    d1, d2 = rand_desc(rng, 255), rand_desc(rng, 256)
    claims = []
    for q in range(128):                                                   # nearest at 2 q + 1, runner-up at 2 q: every train row is somebody's
        d2[2 * q + 1], d2[2 * q] = flipped(d1[q], [q]), flipped(d1[q], [q, q + 1, q + 2])
        claims += [(q, 0, 2 * q + 1, 1), (q, 1, 2 * q, 3)]
    out.append(_case('valu_255x256', d1, d2, _plan(0, 256, 1, 255, 256), claims))
    # 256 x 257: the second chunk holds ONE descriptor, its runner-up key stays kNone
    d1, d2 = rand_desc(rng, 256), rand_desc(rng, 257)
    d1[1] = flipped(d1[0], [200, 201])
    d2[256], d2[0], d2[255] = d1[0], flipped(d1[0], [5]), flipped(d1[1], [10])
    out.append(_case('valu_256x257', d1, d2, _plan(0, 256, 2, 256, 257),
                     [(0, 0, 256, 0), (0, 1, 0, 1), (1, 0, 255, 1), (1, 1, 256, 2)]))
    # 257 x 513: three chunks; nearest and runner-up at every pair of {0, 255, 256, 511, 512}, ties across the chunk edges
    orders, ties = _all_pairs(5)
    d1, d2, claims = _cluster(rng, 257, 513, [0, 255, 256, 511, 512], orders, ties, _spread(257, 30))
    out.append(_case('valu_257x513', d1, d2, _plan(0, 256, 3, 257, 513), claims))
    # 300 x 1025: five chunks, the last of one descriptor
    orders, ties = _all_pairs(3)
    d1, d2, claims = _cluster(rng, 300, 1025, [0, 1023, 1024], orders, ties, _spread(300, 9))
    out.append(_case('valu_300x1025', d1, d2, _plan(0, 256, 5, 300, 1025), claims))
    # 16384 x 8200 without the MFMA form: chunks of 257 - no multiple of the unroll - and a last chunk of 233
    sp = [0, 256, 257, 513, 514, 7966, 7967, 8199]
    orders = [(a, b) for a in range(8) for b in range(8) if abs(a - b) == 1 or {a, b} == {0, 7}]
    ties = [(a, a + 1) for a in range(7)]
    d1, d2, claims = _cluster(rng, 16384, 8200, sp, orders, ties, _spread(16384, len(orders) + len(ties)))
    out.append(_case('valu_16384x8200_chunk257', d1, d2, _plan(0, 257, 32, 16384, 8200), claims, NO_MFMA))
    # the switch from below: one row of pairs short of 2^24; and n2 < 1024 with more than 2^24 pairs
    orders, ties = _all_pairs(4)
    d1, d2, claims = _cluster(rng, 16383, 1024, [0, 255, 256, 1023], orders, ties, _spread(16383, 18))
    out.append(_case('valu_16383x1024', d1, d2, _plan(0, 256, 4, 16383, 1024), claims))
    d1, d2, claims = _cluster(rng, 16401, 1023, [0, 767, 768, 1022], orders, ties, _spread(16401, 18))
    out.append(_case('valu_16401x1023', d1, d2, _plan(0, 256, 4, 16401, 1023), claims))
    return out


def _mfma_cases(rng):
    out = []
    orders, ties = _all_pairs(4)
    # exactly 2^24 pairs: four chunks of one batch, no padding anywhere
    d1, d2, claims = _cluster(rng, 16384, 1024, [0, 255, 256, 1023], orders, ties, _spread(16384, 18))
    out.append(_case('mfma_16384x1024', d1, d2, _plan(1, 256, 4, 16384, 1024), claims))
    # a query block with one real row: that row's query is planted
    d1, d2, claims = _cluster(rng, 16385, 1024, [0, 511, 512, 1023], orders, ties, [16384] + _spread(16384, 17))
    out.append(_case('mfma_16385x1024', d1, d2, _plan(1, 256, 4, 16640, 1024), claims))
    # chunks of 2, 2, 1 batches; the last batch is ONE real descriptor and 255 padding rows
    orders, ties = _all_pairs(5)
    d1, d2, claims = _cluster(rng, 32768, 1025, [0, 511, 512, 1023, 1024], orders, ties, _spread(32768, 30))
    out.append(_case('mfma_32768x1025', d1, d2, _plan(1, 512, 3, 32768, 1280), claims))
    # both sets ragged
    d1, d2, claims = _cluster(rng, 8193, 2049, [0, 255, 256, 2047, 2048], orders, ties, [8192] + _spread(8192, 29))
    out.append(_case('mfma_8193x2049', d1, d2, _plan(1, 256, 9, 8448, 2304), claims))
    return out


def _extreme_cases(rng, form, n1, n2, plan):
    """The extremes of the key range and of the tiles, for one form."""
    out = []
    ones = np.full((n2, 32), 255, dtype=np.uint8)
    pop = lambda d: np.unpackbits(d, axis=1).sum(axis=1).astype(int)
    # every train descriptor all ones: a zero query is 256 from both (the top of the key range), a ones query 0 from both;
    # the train descriptors are identical, so indices 0, 1 for EVERY query
    d1 = rand_desc(rng, n1)
    d1[0], d1[1], d1[n1 - 1], d1[n1 - 2] = 0, 255, 0, 255
    far = 256 - pop(d1)
    claims = [(q, s, s, int(far[q])) for q in _asserted(n1, []) for s in (0, 1)]
    out.append(_case(form + '_all_ones_train', d1, ones, plan, claims))
    # every train descriptor the same random string
    d1, t = rand_desc(rng, n1), rand_desc(rng, 1)
    d1[3], d1[n1 - 3] = t[0], ~t[0]
    dd = pop(d1 ^ t)
    claims = [(q, s, s, int(dd[q])) for q in _asserted(n1, []) for s in (0, 1)]
    out.append(_case(form + '_identical_train', d1, np.repeat(t, n2, axis=0), plan, claims))
    # a query equals train j for j at both ends of every 16-column tile of the first and of the last batch of 256
    d1, d2 = rand_desc(rng, n1), rand_desc(rng, n2)
    last = (n2 - 1) // 256 * 256
    js = [j for b in sorted({0, last}) for t in range(16) for j in (b + 16 * t, b + 16 * t + 15) if j < n2]
    qs = _spread(n1, len(js))
    claims = []
    for q, j in zip(qs, js):
        d1[q] = d2[j]
        claims.append((q, 0, j, 0))
    out.append(_case(form + '_tile_ends', d1, d2, plan, claims))
    # distances 0 and 1; 1 and 1 (a tie: the smaller index first), in a random background
    d1, d2 = rand_desc(rng, n1), rand_desc(rng, n2)
    b0, b1 = rand_desc(rng, 2)
    ja, jb, jc, jd = n2 - 1, 0, 17, n2 - 2
    d2[ja], d2[jb] = b0, flipped(b0, [77])
    d2[jc], d2[jd] = b1, flipped(b1, [3, 4])
    qa, qb = (0, n1 - 1) if n1 > 1 else (0, 0)
    d1[qa] = b0
    d1[qb] = flipped(b1, [3])
    out.append(_case(form + '_dist_0_1_and_1_1', d1, d2, plan,
                     [(qa, 0, ja, 0), (qa, 1, jb, 1), (qb, 0, jc, 1), (qb, 1, jd, 1)]))
    # distances 255 and 256: a zero query, every train descriptor all ones but the last, which has one zero bit
    d1 = rand_desc(rng, n1)
    d1[n1 // 2] = 0
    d2 = ones.copy()
    d2[n2 - 1] = flipped(d2[n2 - 1], [131])
    out.append(_case(form + '_dist_255_256', d1, d2, plan, [(n1 // 2, 0, n2 - 1, 255), (n1 // 2, 1, 0, 256)]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261021)
    out = _valu_cases(rng) + _mfma_cases(rng)
    out += _extreme_cases(rng, 'valu', 257, 513, _plan(0, 256, 3, 257, 513))
    out += _extreme_cases(rng, 'mfma', 16384, 1024, _plan(1, 256, 4, 16384, 1024))
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        c['d1'].setflags(write=False)
        c['d2'].setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c['name'] == name)


def names(form=None):
    return [c['name'] for c in cases() if form is None or c['plan']['mfma'] == (form == 'mfma')]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(asserted queries, idx, dist) of a case by oracle/ft_oracle.py, computed once: the NumPy scan, and up to 300 x 600 the
    pure-Python loops as well, which must agree."""
    from oracle import ft_oracle as fo
    c = case(name)
    sel = c['asserted']
    idx, dist = fo.knn2(c['d1'][sel], c['d2'])
    if len(c['d1']) <= 300 and len(c['d2']) <= 600:
        lidx, ldist = fo.knn2_loops(c['d1'], c['d2'])
        np.testing.assert_array_equal(idx, lidx)
        np.testing.assert_array_equal(dist, ldist)
    for a in (idx, dist):
        a.setflags(write=False)
    return sel, idx, dist
