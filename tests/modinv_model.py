"""Integer restatement of the divstep inversion (mina_bridge_amd/csrc/fe_modinv.cuh), limb by limb: nine signed 30-bit limbs, 64-bit accumulators, the batch of 30
divsteps on the low 30 bits with 32-bit wrapping words, the two matrix updates and the last normalisation, each as the header writes it.  Every step asserts what
the header's comments claim:

    both divisions by 2^30 are exact;                         the matrix entries satisfy |u| + |v| <= 2^30 and |q| + |r| <= 2^30;
    -2p < d, e < p after every batch (THE INVARIANT);         every 64-bit accumulator stays below 2^62 in magnitude (the header's bound; 2^63 is the type's);
    limbs 0..7 of f, g, d, e lie in [0, 2^30) after every update, and every 32-bit signed value fits;
    d a = f and e a = g (mod p) after every batch;            g = 0 within MI_BATCHES = 25 batches.

`inverse_words` returns the inverse of the integer and the trace (delta, f, g, d, e as limb lists) at the end of every batch that ran: what
tests/fuzz/modinv_twin.cpp prints for the compiled header.  `fe_inv_gcd` is the Montgomery-domain routine.  `batch_reference` is the divstep definition on whole
integers: the matrix of a batch must not depend on anything but the low 30 bits."""
import random

P = {0: 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 1: 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001}
R = 1 << 256
BATCHES, STEPS, M30, M32 = 25, 30, (1 << 30) - 1, (1 << 32) - 1
ACC_BOUND = 1 << 62


def s32(x):
    """a 32-bit word read as signed"""
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def fits32(x):
    assert -(1 << 31) <= x < (1 << 31), x
    return x


def acc(x):
    assert abs(x) < ACC_BOUND, x
    return x


def p_limbs(p):
    return [(p >> (30 * i)) & M30 for i in range(9)]


def p_inv30(p):
    x = 1
    for _ in range(5):
        x = x * (2 - (p & M32) * x) & M32
    assert (x * p) & M30 == 1
    return x & M30


def from_words(a):
    assert 0 <= a < R
    return [(a >> (30 * i)) & M30 for i in range(9)]


def value(limbs):
    return sum(v << (30 * i) for i, v in enumerate(limbs))


def divsteps30(delta, f0, g0):
    """mi_divsteps30: unsigned 32-bit words, masks"""
    u, v, q, r, f, g, dl = 1, 0, 0, 1, f0 & M32, g0 & M32, delta & M32
    for _ in range(STEPS):
        c1 = M32 if s32(dl) > 0 else 0
        c2 = M32 if g & 1 else 0
        x, y, z = ((f ^ c1) - c1) & M32, ((u ^ c1) - c1) & M32, ((v ^ c1) - c1) & M32
        g = (g + (x & c2)) & M32; q = (q + (y & c2)) & M32; r = (r + (z & c2)) & M32
        c1 &= c2
        dl = (((dl ^ c1) - c1) + 1) & M32
        f = (f + (g & c1)) & M32; u = (u + (q & c1)) & M32; v = (v + (r & c1)) & M32
        g >>= 1; u = (u << 1) & M32; v = (v << 1) & M32
    t = tuple(s32(x) for x in (u, v, q, r))
    assert abs(t[0]) + abs(t[1]) <= 1 << 30 and abs(t[2]) + abs(t[3]) <= 1 << 30, t
    return s32(dl), t


def batch_reference(delta, f, g):
    """30 divsteps by their definition, on whole (signed) integers -> (delta, (u, v, q, r))"""
    u, v, q, r = 1, 0, 0, 1
    for _ in range(STEPS):
        if delta > 0 and g & 1:
            delta, f, g, u, v, q, r = 1 - delta, g, (g - f) >> 1, 2 * q, 2 * r, q - u, r - v
        elif g & 1:
            delta, g, u, v, q, r = 1 + delta, (g + f) >> 1, 2 * u, 2 * v, q + u, r + v
        else:
            delta, g, u, v = 1 + delta, g >> 1, 2 * u, 2 * v
    return delta, (u, v, q, r)


def _shift30(c):
    return c >> 30                                                # mi_sar: floor(c / 2^30)


def update_fg(f, g, t):
    u, v, q, r = t
    cf, cg = acc(u * f[0] + v * g[0]), acc(q * f[0] + r * g[0])
    assert cf & M30 == 0 and cg & M30 == 0, "the division of (f, g) is exact"
    cf, cg = _shift30(cf), _shift30(cg)
    nf, ng = [0] * 9, [0] * 9
    for i in range(1, 9):
        cf = acc(cf + u * f[i] + v * g[i]); cg = acc(cg + q * f[i] + r * g[i])
        nf[i - 1] = cf & M30; cf = _shift30(cf)
        ng[i - 1] = cg & M30; cg = _shift30(cg)
    nf[8], ng[8] = fits32(cf), fits32(cg)
    return nf, ng


def update_de(p, d, e, t):
    u, v, q, r = t
    pl, pinv = p_limbs(p), p_inv30(p)
    sd, se = (-1 if d[8] < 0 else 0), (-1 if e[8] < 0 else 0)
    md, me = fits32((u & sd) + (v & se)), fits32((q & sd) + (r & se))
    cd, ce = acc(u * d[0] + v * e[0]), acc(q * d[0] + r * e[0])
    md = fits32(md - ((pinv * (cd & M32) + (md & M32)) & M30))
    me = fits32(me - ((pinv * (ce & M32) + (me & M32)) & M30))
    assert -(1 << 31) < md <= 1 << 30 and -(1 << 31) < me <= 1 << 30
    cd = acc(cd + pl[0] * md); ce = acc(ce + pl[0] * me)
    assert cd & M30 == 0 and ce & M30 == 0, "the division of (d, e) is exact"
    cd, ce = _shift30(cd), _shift30(ce)
    nd, ne = [0] * 9, [0] * 9
    for i in range(1, 9):
        cd = acc(cd + u * d[i] + v * e[i]); ce = acc(ce + q * d[i] + r * e[i])
        if pl[i]:
            cd = acc(cd + pl[i] * md); ce = acc(ce + pl[i] * me)
        nd[i - 1] = cd & M30; cd = _shift30(cd)
        ne[i - 1] = ce & M30; ce = _shift30(ce)
    nd[8], ne[8] = fits32(cd), fits32(ce)
    return nd, ne


def normalize(p, d, f_top):
    pl = p_limbs(p)
    add, neg = (-1 if d[8] < 0 else 0), (-1 if f_top < 0 else 0)
    out, c = list(d), 0
    for i in range(9):
        x = fits32(out[i] + (pl[i] & add))
        x = fits32((x ^ neg) - neg)
        x = fits32(x + c)
        c = x >> 30
        out[i] = x & M30 if i < 8 else x
    assert -p < value(out) < p
    add2, c = (-1 if out[8] < 0 else 0), 0
    for i in range(9):
        x = fits32(out[i] + (pl[i] & add2) + c)
        c = x >> 30
        out[i] = x & M30 if i < 8 else x
    assert 0 <= value(out) < p and all(0 <= v <= M30 for v in out)
    return out


def to_words(limbs):
    w = []
    for i in range(8):
        k, s = (32 * i) // 30, (32 * i) % 30
        w.append(((limbs[k] >> s) | (limbs[k + 1] << (30 - s))) & M32)
    return sum(x << (32 * i) for i, x in enumerate(w))


def inverse_words(F, a, stats=None):
    """mi_inverse_words: the inverse of the integer a (0 for a = 0 mod p) and the trace [(delta, f, g, d, e)] of the batches that ran"""
    p = P[F]
    f, g, d, e, delta, trace = p_limbs(p), from_words(a), [0] * 9, [1] + [0] * 8, 1, []
    for _ in range(BATCHES):
        if not any(g):
            break
        delta, t = divsteps30(delta, f[0], g[0])
        assert (delta, t) == batch_reference(trace[-1][0] if trace else 1, value(f), value(g)), "the matrix is a function of the low 30 bits"
        d, e = update_de(p, d, e, t)
        f, g = update_fg(f, g, t)
        for x in (f, g, d, e):
            assert all(0 <= v <= M30 for v in x[:8])
        vf, vg, vd, ve = value(f), value(g), value(d), value(e)
        assert -2 * p < vd < p and -2 * p < ve < p, "the invariant of d, e"
        assert abs(vf) < R and abs(vg) < R and vf & 1
        assert (vd * a - vf) % p == 0 and (ve * a - vg) % p == 0
        trace.append((delta, list(f), list(g), list(d), list(e)))
    assert not any(g), "g = 0 within 25 batches"
    assert abs(value(f)) == (1 if a % p else p)
    if stats is not None:
        stats[len(trace)] = stats.get(len(trace), 0) + 1
    return to_words(normalize(p, d, f[8])), trace


def fe_inv_gcd(F, a, stats=None):
    """Montgomery words below p in, the Montgomery words of the inverse out"""
    p = P[F]
    x, _ = inverse_words(F, a, stats)
    rinv, r2 = pow(R, -1, p), R * R % p
    mm = lambda s, t: s * t * rinv % p
    return mm(mm(x, r2), r2)


# ------------------------------------------------------------------------------------------------ the same routine on many inputs at once (numpy, int64 lanes)
def _sign_of(x):
    """limbs 0..7 in [0, 2^30), limb 8 signed -> the sign of the value per lane (-1, 0, 1)"""
    import numpy as np
    low = (x[:8] != 0).any(axis=0)
    return np.where(x[8] < 0, -1, np.where((x[8] > 0) | low, 1, 0))


def _carry(x):
    import numpy as np
    out, c = x.copy(), np.zeros_like(x[0])
    for i in range(9):
        t = out[i] + c
        c = t >> 30
        out[i] = t & M30 if i < 8 else t
    return out


def inverse_words_many(F, xs):
    """`inverse_words` with one input per numpy lane: the same statements on int64 arrays.  int64 wraps silently, so every accumulator's bound is asserted TWICE:
    on its operands before the sum (matrix rows <= 2^30, limbs <= 2^30, the carry below 2^33, |md| < 2^31: the sum cannot wrap) and on the sum.
    -> ([inverse per input], [batches per input])"""
    import numpy as np
    p, n = P[F], len(xs)
    pl, pinv = p_limbs(p), p_inv30(p)
    col = lambda limbs: np.array(limbs, np.int64).reshape(9, 1)
    f = np.repeat(col(pl), n, axis=1)
    g = np.array([from_words(x) for x in xs], np.int64).T.copy()
    d, e = np.zeros((9, n), np.int64), np.zeros((9, n), np.int64)
    e[0] = 1
    delta, batches = np.ones(n, np.int64), np.zeros(n, np.int64)
    m32 = np.int64(M32)
    sx = lambda w: np.where(w >> 31 != 0, w - (1 << 32), w)      # a 32-bit word (held in int64) read as signed

    def lanes(live, new, old):
        return np.where(live, new, old)

    def bounded(c, u, x, v, y):
        assert (np.abs(c) < 1 << 34).all() and (np.abs(u) + np.abs(v) <= 1 << 30).all() and (np.abs(x) <= 1 << 30).all() and (np.abs(y) <= 1 << 30).all()
        s = c + u * x + v * y
        assert (np.abs(s) < ACC_BOUND).all()
        return s
    for _ in range(BATCHES):
        live = (g != 0).any(axis=0)
        if not live.any():
            break
        batches += live
        # mi_divsteps30
        u, v, q, r = np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64)
        ff, gg, dl = f[0] & m32, g[0] & m32, delta & m32
        for _ in range(STEPS):
            c1 = np.where(sx(dl) > 0, m32, 0)
            c2 = np.where(gg & 1 != 0, m32, 0)
            x, y, z = ((ff ^ c1) - c1) & m32, ((u ^ c1) - c1) & m32, ((v ^ c1) - c1) & m32
            gg = (gg + (x & c2)) & m32; q = (q + (y & c2)) & m32; r = (r + (z & c2)) & m32
            c1 &= c2
            dl = (((dl ^ c1) - c1) + 1) & m32
            ff = (ff + (gg & c1)) & m32; u = (u + (q & c1)) & m32; v = (v + (r & c1)) & m32
            gg >>= 1; u = (u << 1) & m32; v = (v << 1) & m32
        u, v, q, r = sx(u), sx(v), sx(q), sx(r)
        assert (np.abs(u) + np.abs(v) <= 1 << 30).all() and (np.abs(q) + np.abs(r) <= 1 << 30).all()
        # mi_update_de
        sd, se = np.where(d[8] < 0, -1, 0), np.where(e[8] < 0, -1, 0)
        md, me = (u & sd) + (v & se), (q & sd) + (r & se)
        zero = np.zeros(n, np.int64)
        cd, ce = bounded(zero, u, d[0], v, e[0]), bounded(zero, q, d[0], r, e[0])
        md = md - ((pinv * (cd & m32) + (md & m32)) & M30)
        me = me - ((pinv * (ce & m32) + (me & m32)) & M30)
        assert ((md > -(1 << 31)) & (md <= 1 << 30) & (me > -(1 << 31)) & (me <= 1 << 30)).all()
        cd = cd + pl[0] * md; ce = ce + pl[0] * me
        assert ((cd & M30) == 0).all() and ((ce & M30) == 0).all(), "the division of (d, e) is exact"
        cd >>= 30; ce >>= 30
        nd, ne = np.zeros_like(d), np.zeros_like(e)
        for i in range(1, 9):
            cd = bounded(cd, u, d[i], v, e[i]); ce = bounded(ce, q, d[i], r, e[i])
            if pl[i]:
                cd = cd + pl[i] * md; ce = ce + pl[i] * me                   # < 2^30 * 2^31 on top of a sum below 2^61 + 2^34
                assert (np.abs(cd) < ACC_BOUND).all() and (np.abs(ce) < ACC_BOUND).all()
            nd[i - 1] = cd & M30; cd >>= 30
            ne[i - 1] = ce & M30; ce >>= 30
        nd[8], ne[8] = cd, ce
        # mi_update_fg
        cf, cg = bounded(zero, u, f[0], v, g[0]), bounded(zero, q, f[0], r, g[0])
        assert ((cf & M30) == 0).all() and ((cg & M30) == 0).all(), "the division of (f, g) is exact"
        cf >>= 30; cg >>= 30
        nf, ng = np.zeros_like(f), np.zeros_like(g)
        for i in range(1, 9):
            cf = bounded(cf, u, f[i], v, g[i]); cg = bounded(cg, q, f[i], r, g[i])
            nf[i - 1] = cf & M30; cf >>= 30
            ng[i - 1] = cg & M30; cg >>= 30
        nf[8], ng[8] = cf, cg
        for x in (nf, ng, nd, ne):
            assert (np.abs(x[8]) < 1 << 17).all()
        # -2p < d, e < p:  d + 2p > 0 and p - d > 0, limb by limb
        for x in (nd, ne):
            assert (_sign_of(_carry(x + 2 * col(pl))) > 0).all() and (_sign_of(_carry(col(pl) - x)) > 0).all(), "the invariant of d, e"
        f, g, d, e, delta = lanes(live, nf, f), lanes(live, ng, g), lanes(live, nd, d), lanes(live, ne, e), lanes(live, sx(dl), delta)
    assert not (g != 0).any(), "g = 0 within 25 batches"
    out = [to_words(normalize(p, [int(v) for v in d[:, j]], int(f[8, j]))) for j in range(n)]
    return out, [int(b) for b in batches]


def corners(F):
    """the named inputs every tier runs (plain integers below p; the Montgomery tiers convert)"""
    p = P[F]
    xs = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 254) - 1, 1 << 254, (1 << 255) % p, (1 << 256) % p, (1 << 30) - 1, 1 << 30, (1 << 60) + 1,
          pow(5, (p - 1) >> 32, p)]
    assert all(0 <= x < p for x in xs)
    return xs


def sized(F, count, seed="modinv/sized"):
    """`count` values of each of 31, 32, 33, 61, 128 and 129 bits"""
    rng = random.Random(f"{seed}/{F}")
    return [rng.getrandbits(k - 1) | (1 << (k - 1)) for k in (31, 32, 33, 61, 128, 129) for _ in range(count)]


def randoms(F, count, seed="modinv/random"):
    rng = random.Random(f"{seed}/{F}")
    return [rng.randrange(P[F]) for _ in range(count)]
