"""The divstep inversion on integers (tests/modinv_model.py, the limb-by-limb restatement of mina_bridge_amd/csrc/fe_modinv.cuh) against pow(x, p - 2, p) for both
Pasta primes: the named corners, values of 31 .. 129 bits and 20 000 seeded random values.  The model asserts on every input that both divisions are exact, the
matrix entries are at most 2^30, -2p < d, e < p, every accumulator is below 2^62 (the header's bound; the type's is 2^63), the batch matrix is that of the divstep
definition on the whole integers (so: a function of the low 30 bits alone) and g = 0 within 25 batches."""
import random

import pytest

import modinv_model as M


@pytest.mark.parametrize("F", [0, 1])
def test_constants(F):
    p = M.P[F]
    assert M.value(M.p_limbs(p)) == p and M.p_limbs(p)[8] == 1 << 14 and M.p_limbs(p)[5:8] == [0, 0, 0]
    assert M.p_inv30(p) * p % (1 << 30) == 1
    assert (49 * 256 + 57) // 17 == 741 < M.BATCHES * M.STEPS


@pytest.mark.parametrize("F", [0, 1])
def test_corners_and_sized_values(F):
    p, stats = M.P[F], {}
    xs = M.corners(F) + M.sized(F, 40)
    assert len(M.corners(F)) == 16
    for x in xs:
        got, trace = M.inverse_words(F, x, stats)
        assert got == pow(x, p - 2, p), hex(x)
        assert len(trace) <= M.BATCHES
    assert M.inverse_words(F, 0)[0] == 0 and M.inverse_words(F, 0)[1] == []
    assert M.inverse_words(F, 1)[0] == 1
    print(sorted(stats.items()))


@pytest.mark.parametrize("F", [0, 1])
def test_montgomery_form_is_fe_inv(F):
    """fe_inv_gcd: Montgomery words in and out, 0 -> 0, below p"""
    p = M.P[F]
    for x in M.corners(F) + M.randoms(F, 50, "modinv/mont"):
        a = x * M.R % p
        got = M.fe_inv_gcd(F, a)
        assert got == pow(x, p - 2, p) * M.R % p and 0 <= got < p


@pytest.mark.parametrize("F", [0, 1])
def test_twenty_thousand_random_values(F):
    p = M.P[F]
    xs = M.randoms(F, 20000)
    got, batches = M.inverse_words_many(F, xs)
    bad = [hex(x) for x, r in zip(xs, got) if r != pow(x, p - 2, p)]
    assert not bad, bad[:3]
    hist = {b: batches.count(b) for b in sorted(set(batches))}
    print(hist)
    assert max(batches) <= M.BATCHES


@pytest.mark.parametrize("F", [0, 1])
def test_the_lanes_and_the_scalar_model_agree(F):
    xs = M.corners(F) + M.sized(F, 5) + M.randoms(F, 100, "modinv/both")
    got, batches = M.inverse_words_many(F, xs)
    for x, r, b in zip(xs, got, batches):
        want, trace = M.inverse_words(F, x)
        assert (r, b) == (want, len(trace)), hex(x)


def test_the_batch_matrix_depends_on_the_low_30_bits_only():
    rng = random.Random("modinv/low30")
    for _ in range(2000):
        f, g = rng.getrandbits(256) | 1, rng.getrandbits(256)
        if rng.random() < .5: f = -f
        if rng.random() < .5: g = -g
        delta = rng.randint(-40, 40)
        whole = M.batch_reference(delta, f, g)
        assert M.divsteps30(delta, f & M.M30, g & M.M30) == whole
        assert M.divsteps30(delta, (f & M.M30) | (rng.getrandbits(2) << 30), (g & M.M30) | (rng.getrandbits(2) << 30)) == whole      # bits 30, 31 of the words are not read


@pytest.mark.parametrize("F", [0, 1])
def test_the_invariant_holds_from_its_extremes(F):
    """d, e at the ends of (-2p, p) under matrices at the ends of |u| + |v| <= 2^30: the update stays inside and below the accumulator bound"""
    p = M.P[F]
    signed = lambda x: M.from_words(x % M.R)[:8] + [x >> 240]
    ends = [-2 * p + 1, -p - 1, -p, -p + 1, -1, 0, 1, p - 1]
    one = 1 << 30
    mats = [(one, 0, 0, one), (-one, 0, 0, -one), (0, one, -one, 0), (0, -one, one, 0), (one // 2, one // 2, -one // 2, one // 2), (one - 1, -1, 1, -(one - 1))]
    for dv in ends:
        for ev in ends:
            for t in mats:
                d, e = signed(dv), signed(ev)
                assert M.value(d) == dv and M.value(e) == ev
                nd, ne = M.update_de(p, d, e, t)
                vd, ve = M.value(nd), M.value(ne)
                assert -2 * p < vd < p and -2 * p < ve < p
                assert (vd * one - (t[0] * dv + t[1] * ev)) % p == 0 and (ve * one - (t[2] * dv + t[3] * ev)) % p == 0
