"""shared by the crafted-SRS tests: the reference's SRS file format, SRSs whose Lagrange basis is a list of KNOWN multiples of one point, the big-int
reference of a public-input commitment on such an SRS, and a big-int model of the digit walk of the direct commitment kernels (lagrange.cuh) that says
which inputs meet the group law's exceptional cases.

The construction: a base point G and scalars c_0 .. c_{n-1};  a_j = sum_i c_i w^(ij) mod r,  g_j = a_j G.  The Lagrange basis of g[0..n) is then exactly
L_i = (1/n) sum_j w^(-ij) g_j = c_i G, so  public_comm = h - sum_i pub_i L_i = (t - sum_i pub_i c_i) G  for h = t G: one dot product and one scalar
multiplication.  Equal c's are equal basis points, opposite c's opposite ones, c_i = 0 a basis point at infinity."""
import random
import struct

import numpy as np

DEPTH, LOG2_DOMAIN, NPUB, NPUB_SMALL = 256, 6, 32, 5


def srs_blob(oracle, curve, g, h):
    """SRS{g, h} in the reference's file format: fixarray(2)[ array32(n)[bin8(33) ...], bin8(33) ]"""
    comp = oracle.point_compress(curve, np.concatenate([g, h.reshape(1, 64)]))
    body = b"".join(b"\xc4\x21" + comp[i].tobytes() for i in range(len(g)))
    return b"\x92" + b"\xdd" + struct.pack(">I", len(g)) + body + b"\xc4\x21" + comp[len(g)].tobytes()


def scalar_modulus(curve):
    from oracle import pasta_ref as R
    return R.scalar_modulus(curve)


def domain_root(r, log2_domain):
    from oracle import pasta_ref as R
    return pow(R.two_adic_root_of_unity(r), 1 << (32 - log2_domain), r)


def point_mul(oracle, curve, G, k):
    """(k mod r) G as 64 bytes (zeros = infinity), by the oracle's naive sum over the one point"""
    k %= scalar_modulus(curve)
    if k == 0:
        return np.zeros(64, np.uint8)
    return oracle.msm_naive(curve, np.asarray(G, np.uint8).reshape(1, 64), oracle.int_to_le(k).reshape(1, 32))


def s1_coefficients(curve, seed=606):
    """S1: L_0 = L_1 = L_8 = G, L_2 = L_16 = -G, L_4 = 2 G, L_3 = L_24 = infinity, every other one a random non-zero multiple.  Indices 0, 8, 16, 24 are one
    lane's scalars in the 8-lanes-per-proof form; indices 0 .. 4 carry the same relations for 5 public inputs."""
    r = scalar_modulus(curve)
    rng = random.Random(seed + curve)
    c = [rng.randrange(1, r) for _ in range(1 << LOG2_DOMAIN)]
    c[0] = c[1] = 1; c[2] = r - 1; c[3] = 0; c[4] = 2; c[8] = 1; c[16] = r - 1; c[24] = 0
    return c


def s2_coefficients():
    """S2: c = e_0 -- every g_j = G, L_0 = G and every other basis point is infinity"""
    return [1] + [0] * ((1 << LOG2_DOMAIN) - 1)


def blinder(curve, seed=707):
    return random.Random(seed + curve).randrange(1, scalar_modulus(curve))


def structured_srs(oracle, curve, c, t):
    """-> (g [DEPTH, 64], h [64], G [64]): g_j = (sum_i c_i w^(ij)) G over the domain of len(c) points, the honest points behind them, h = t G.  G is the honest
    SRS' first point (not itself part of the crafted SRS)."""
    r = scalar_modulus(curve)
    n = len(c)
    k = n.bit_length() - 1
    assert n == 1 << k and n <= DEPTH
    w = domain_root(r, k)
    wp = [pow(w, e, r) for e in range(n)]
    a = [sum(c[i] * wp[(i * j) % n] for i in range(n)) % r for j in range(n)]
    assert all(a), "a crafted SRS point would be infinity: the file format has no encoding for it"
    honest, _ = oracle.srs_create(curve, DEPTH, threads=4)
    G = honest[0].copy()
    g = honest.copy()
    for j in range(n):
        g[j] = point_mul(oracle, curve, G, a[j])
    return g, point_mul(oracle, curve, G, t), G


def reference_commitment(oracle, curve, c, t, G, pubs):
    """h - (sum_i pub_i c_i mod r) G as 64 bytes: big-int dot product, one scalar multiplication, affine add / neg of the Python restatement"""
    from oracle import pasta_ref as R
    r, m = scalar_modulus(curve), R.base_modulus(curve)
    s = sum(p * ci for p, ci in zip(pubs, c)) % r
    A = oracle.bytes_to_point(point_mul(oracle, curve, G, s))
    H = oracle.bytes_to_point(point_mul(oracle, curve, G, t))
    return oracle.point_to_bytes(R.add(H, R.neg(A, m), m))


# ---------------------------------------------------------------- the digit walk of the direct commitment kernels, on multiples of G
def signed_digits(s):
    """the kernels' recoding of a scalar below 2^255: 32 base-256 digits, a digit above 128 negated with a carry into the next window (128 itself stays)"""
    assert 0 <= s < 1 << 255
    out, carry = [], 0
    for w in range(32):
        d = ((s >> (8 * w)) & 0xFF) + carry
        carry = 1 if d > 128 else 0
        out.append(d - 256 if carry else d)
    assert carry == 0 and sum(d << (8 * w) for w, d in enumerate(out)) == s
    return out


def prefix_below(s, w):
    """what the walk has added of scalar s (as a multiple of its basis point) before it reaches window w"""
    return sum(d << (8 * v) for v, d in enumerate(signed_digits(s)[:w]))


def _meet(acc, term, r):
    if acc % r == 0 or term % r == 0:
        return None
    if (acc - term) % r == 0:
        return "equal"
    if (acc + term) % r == 0:
        return "opposite"
    return None


def walk(c, pubs, lanes_per_proof, r):
    """One proof through pubcomm_direct*_kernel<F, lanes_per_proof>, every point a multiple of G mod r (0 = infinity).  Lane l adds, for the scalars i = l, l + lanes, ...
    in turn and the windows of each from the lowest, digit * 256^w * c_i G into its running sum (zero digits and basis points at infinity are skipped); the lanes' sums
    are then added pairwise, lane l taking lane l + d for d = lanes/2 .. 1.  Returns
      steps: [(kind, i, w, lane)]  the running sum was +- the point about to be added (kind "equal" / "opposite") at scalar i, window w
      tree:  [(kind, d, lane)]     the same between two partial sums, at the levels and lanes that reach lane 0
      pairs: [(kind, l1, l2)]      lanes whose final sums are equal or opposite
      sums, total                  the lanes' final sums and the proof's, as multiples of G"""
    lanes = lanes_per_proof
    steps, sums = [], []
    for l in range(lanes):
        acc = 0
        for i in range(l, len(pubs), lanes):
            if c[i] % r == 0:
                continue
            for w, d in enumerate(signed_digits(pubs[i])):
                if d == 0:
                    continue
                term = (d << (8 * w)) * c[i] % r
                kind = _meet(acc, term, r)
                if kind:
                    steps.append((kind, i, w, l))
                acc = (acc + term) % r
        sums.append(acc)
    pairs = [(k, a, b) for a in range(lanes) for b in range(a + 1, lanes) for k in [_meet(sums[a], sums[b], r)] if k]
    tree, cur, d = [], list(sums), lanes // 2
    while d >= 1:
        for l in range(d):
            kind = _meet(cur[l], cur[l + d], r)
            if kind:
                tree.append((kind, d, l))
        cur = [(cur[l] + cur[l + d]) % r if l + d < lanes else cur[l] for l in range(lanes)]
        d //= 2
    assert cur[0] == sum(sums) % r == sum(p * ci for p, ci in zip(pubs, c)) % r
    return {"steps": steps, "tree": tree, "pairs": pairs, "sums": sums, "total": cur[0]}


# ---------------------------------------------------------------- the rows of public inputs on S1
MID = 3 * 256 ** 2


def s1_cases(curve, c, t):
    """name -> dict(pubs = NPUB scalars, and what the row claims to meet: steps8 / tree64 = entries walk() must report in the 8- and 64-lane form, `clean` = it must
    report nothing at all, `total` = the sum as a multiple of G).  The names ending in _top carry random scalars in the other positions."""
    r = scalar_modulus(curve)
    rng = random.Random(808 + curve)
    rand = lambda: rng.randrange(1, r)
    sparse = lambda d: [d.get(i, 0) for i in range(NPUB)]
    dense = lambda d, zero=(): [d[i] if i in d else 0 if i in zero else rand() for i in range(NPUB)]

    def solved(target, free=5):
        """random scalars everywhere, position `free` solved for sum_i pub_i c_i = target"""
        p = dense({free: 0})
        p[free] = (target - sum(x * ci for x, ci in zip(p, c))) * pow(c[free], r - 2, r) % r
        return p

    second_neg = MID + 0xF9                                        # digits -7, +1 (the carry), +3
    first_neg = MID - prefix_below(second_neg, 2)                  # ... so that the sum stands at 3 * 256^2 G when window 2 adds exactly that
    first_carry = 256 - prefix_below(second_neg, 1)                # ... and at 256 G when window 1 (nothing but the carry) adds that
    big = [r, r + 5, (1 << 255) - 1, int.from_bytes(b"\x80" * 31 + b"\x7f", "little")]
    large = dense({0: big[0], 1: big[1], 4: big[2], 8: big[3], 9: big[2], 12: big[3], 16: big[1]})
    cases = {
        "equal": dict(pubs=sparse({0: 5, 8: 5}), steps8=[("equal", 8, 0, 0)], tree64=[("equal", 8, 0)], total=10),
        "opposite": dict(pubs=sparse({0: 5, 16: 5}), steps8=[("opposite", 16, 0, 0)], tree64=[("opposite", 16, 0)], total=0),
        "mid": dict(pubs=sparse({0: MID - 7, 8: MID + 7}), steps8=[("equal", 8, 2, 0)]),
        "mid_neg": dict(pubs=sparse({0: first_neg, 8: second_neg}), steps8=[("equal", 8, 2, 0)]),
        "mid_carry": dict(pubs=sparse({0: first_carry, 8: second_neg}), steps8=[("equal", 8, 1, 0)]),
        "inf_basis": dict(pubs=sparse({3: rand(), 24: rand()}), clean=True, total=0),
        "inf_basis_top": dict(pubs=dense({3: rand(), 24: rand()}), clean=True),
        "a_eq_h_one": dict(pubs=sparse({0: t}), clean=True, total=t),
        "a_eq_h": dict(pubs=solved(t), clean=True, total=t),
        "a_eq_neg_h_one": dict(pubs=sparse({0: r - t}), clean=True, total=r - t),
        "a_eq_neg_h": dict(pubs=solved(r - t), clean=True, total=r - t),
        # r G = infinity: the last add of scalar 0 meets the opposite of the running sum; 2^255 - 1 ends in digit 128 with a carry in, 0x7f 80 .. 80 is digit 128 in every window
        "large": dict(pubs=large, steps8=[("opposite", 0, 31, 0)]),
        "large_reduced": dict(pubs=[x % r for x in large]),
        "equal_top": dict(pubs=dense({0: 5, 8: 5}), steps8=[("equal", 8, 0, 0)]),
        "opposite_top": dict(pubs=dense({0: 5, 16: 5})),
        "opposite_top_lane": dict(pubs=dense({0: 5, 16: 5}, zero=(8,)), steps8=[("opposite", 16, 0, 0)]),
        "mid_top": dict(pubs=dense({0: MID - 7, 8: MID + 7}), steps8=[("equal", 8, 2, 0)]),
        "mid_neg_top": dict(pubs=dense({0: first_neg, 8: second_neg}), steps8=[("equal", 8, 2, 0)]),
    }
    for i in range(3):
        cases["control_%d" % i] = dict(pubs=dense({}), clean=True)
    assert signed_digits(big[2])[31] == 128 and signed_digits(big[2])[30] == 0 and set(signed_digits(big[3])[:31]) == {128}
    return cases


def s1_cases_small(curve, c, t):
    """the same relations among indices 0 .. 4, for NPUB_SMALL public inputs: every lane holds one scalar, so the exceptional cases sit in the tree and in the finish"""
    r = scalar_modulus(curve)
    rng = random.Random(909 + curve)
    rand = lambda: rng.randrange(1, r)
    half = pow(2, r - 2, r)                                        # c_4 = 2

    def solved(target):
        p = [rand() for _ in range(4)] + [0]
        p[4] = (target - sum(x * ci for x, ci in zip(p, c))) * half % r
        return p
    return {
        "equal": dict(pubs=[5, 5, 0, 0, 0], tree8=[("equal", 1, 0)], total=10),
        "opposite": dict(pubs=[5, 0, 5, 0, 0], tree8=[("opposite", 2, 0)], total=0),
        "a_eq_h": dict(pubs=solved(t), clean=True, total=t),
        "a_eq_neg_h": dict(pubs=solved(r - t), clean=True, total=r - t),
        "control": dict(pubs=[rand() for _ in range(5)], clean=True),
    }


def rows_le(oracle, cases):
    """the cases' scalars as [rows, npub, 32] bytes, in the dict's order"""
    return np.stack([oracle.ints_to_le(v["pubs"]) for v in cases.values()])
