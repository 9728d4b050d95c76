"""The host restatement of the documented random streams (tests/stream_reference.py) on the CPU: Philox4x32-10 against
Random123's known-answer vectors, the 53-bit uniform's range, and the distributions of the stretch factor and of the
partner index at fixed seeds. tests/test_gpu_sampler_replay.py shows the device bit-equal to this restatement, so the
distributions checked here are the device's."""
import numpy as np
import pytest

import stream_reference as SR

SEED = 0x9E3779B97F4A7C15
N_DRAWS = 100000

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter, key, want", KAT)
def test_philox_known_answers(counter, key, want):
    seed = key[0] | (key[1] << 32)
    got = SR.philox4x32_10(counter, seed)
    assert got == want, [hex(w) for w in got]
    # the array form, the counter broadcast over a batch
    words = SR.philox_words(*[np.full(3, c, dtype=np.uint64) for c in counter], seed)
    assert all(np.all(w == np.uint64(x)) for w, x in zip(words, want))


def test_the_high_key_word_and_every_counter_word_matter():
    base = SR.philox4x32_10((1, 2, 3, 0), SEED)
    assert SR.philox4x32_10((1, 2, 3, 0), SEED & 0xFFFFFFFF) != base
    assert SR.philox4x32_10((1, 2, 3, 0), SEED ^ (1 << 32)) != base
    for k in range(4):
        c = [1, 2, 3, 0]
        c[k] += 1
        assert SR.philox4x32_10(c, SEED) != base


def test_uniform53_range_and_bits():
    top = 0xFFFFFFFF
    assert SR.uniform53(0, 0) == 2.0 ** -54
    assert SR.uniform53(top, top) == 1.0            # 2^53 - 1/2 rounds to 2^53 in fp64
    assert SR.uniform53(top, top - 64) == 1.0 - 2.0 ** -52
    # 27 bits of the first word and 26 of the second, none shared
    assert SR.uniform53(1 << 5, 0) - SR.uniform53(0, 0) == 2.0 ** -27
    assert SR.uniform53(0, 1 << 6) - SR.uniform53(0, 0) == 2.0 ** -53
    assert SR.uniform53(31, 63) == SR.uniform53(0, 0)
    assert float(SR.uniform53(1 << 30, 0)) == 0.25 + 2.0 ** -54
    assert float(SR.uniform53(1 << 31, 0)) == 0.5   # from 2^52 on the half is rounded away (to even)


def draws(half, seed=SEED, gp=3):
    """N_DRAWS draws over steps x walkers of one problem: (z, index of the partner within its half, h)."""
    W = 2 * half
    steps = -(-N_DRAWS // W)
    s = np.arange(steps)[:, None]
    w = np.arange(W)[None, :]
    z, cw = SR.draw(seed, gp, s, w, half, w % 2)
    h = np.broadcast_to(w % 2, cw.shape)
    assert np.all(cw % 2 == 1 - h)
    return z.reshape(-1)[:N_DRAWS], (cw // 2).reshape(-1)[:N_DRAWS]


@pytest.mark.parametrize("seed", [SEED, 11])
def test_stretch_factor_follows_its_distribution(seed):
    """g(z) ~ 1 / sqrt(z) on [1/2, 2] (a = 2): F(z) = sqrt(2 z) - 1. Kolmogorov-Smirnov distance over 1e5 draws below
    1.95 / sqrt(N), the 0.1 % point."""
    z, _ = draws(16, seed)
    assert z.min() > 0.5 and z.max() <= 2.0
    F = np.sqrt(2.0 * np.sort(z)) - 1.0
    i = np.arange(1, z.size + 1)
    d = max(np.max(i / z.size - F), np.max(F - (i - 1) / z.size))
    print("KS distance %.5f bound %.5f" % (d, 1.95 / np.sqrt(z.size)))
    assert d < 1.95 / np.sqrt(z.size)


@pytest.mark.parametrize("half", [3, 128])
def test_every_partner_occurs_and_evenly(half):
    from scipy.stats import chi2
    _, k = draws(half)
    counts = np.bincount(k, minlength=half)
    assert counts.size == half and counts.min() > 0
    c = float(np.sum((counts - N_DRAWS / half) ** 2) / (N_DRAWS / half))
    bound = float(chi2.ppf(0.999, half - 1))
    print("half %d chi2 %.2f bound %.2f" % (half, c, bound))
    assert c < bound


def test_z_and_the_acceptance_uniform_come_from_different_blocks():
    s = np.arange(64)[:, None]
    w = np.arange(8)[None, :]
    z, _ = SR.draw(SEED, 0, s, w, 4, w % 2)
    u = np.sqrt(2.0 * z) - 1.0
    assert not np.any(np.isclose(u, SR.accept_uniform(SEED, 0, s, w), rtol=0, atol=1e-12))


def test_propose_gives_both_roundings():
    rng = np.random.default_rng(5)
    x, c = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    z = rng.uniform(0.5, 2.0, 200)
    plain, fused = SR.propose(x, c, z)
    assert np.array_equal(plain, c - (c - x) * z[:, None])
    assert np.max(np.abs(plain - fused)) <= 2.0 ** -51 * np.max(np.abs(plain)) and np.any(plain != fused)
    # exact cases agree: z = 1 gives x's rounding of c - (c - x)
    p1, f1 = SR.propose(x, c, np.ones(200))
    assert np.array_equal(p1, f1)


def test_scan64_is_the_doubling_order():
    rng = np.random.default_rng(6)
    x = rng.exponential(size=64)
    y = SR.scan64(x)
    assert np.allclose(y, np.cumsum(x), rtol=1e-14) and y[0] == x[0] and y[1] == x[0] + x[1]
    # lane 3 = (x0 + x1) + (x2 + x3), not ((x0 + x1) + x2) + x3
    assert y[3] == (x[2] + x[3]) + (x[0] + x[1])


# ------------------------------------------------------------------ the chain replay holds a host sampler to the stream
def gaussian(D):
    rng = np.random.default_rng(40 + D)
    A = rng.normal(size=(D, D))
    prec = A @ A.T + D * np.eye(D)

    def logp(p):
        p = np.atleast_2d(p)
        return -0.5 * np.einsum("pi,ij,pj->p", p, prec, p) - 300.0
    return logp, 1.0 / np.sqrt(np.diag(prec))


def host_case(D, W, steps, seed=SEED, gp=2, box=4.0, **broken):
    logp, sig = gaussian(D)
    rng = np.random.default_rng(W)
    lo, hi = -box * sig, box * sig
    p0 = rng.uniform(-2, 2, (W, D)) * sig
    return (logp, lo, hi, p0) + SR.host_chain(logp, p0, lo, hi, steps, seed, gp, **broken)


@pytest.mark.parametrize("D, W", [(1, 2), (2, 6), (7, 16)])
def test_replay_accepts_the_documented_sampler(D, W):
    logp, lo, hi, p0, chain, lp, acc = host_case(D, W, 40, box=1.5)
    r = SR.replay_chain(chain, lp, acc, p0, lo, hi, SEED, 2, lambda v: -logp(v))
    print(D, W, r.decisions, r.n_accepted, r.n_box, r.n_nonfinite, r.n_ambiguous, r.found)
    assert "plain" in r.found and r.n_ambiguous == 0
    assert 0.1 * r.decisions <= r.n_accepted <= 0.9 * r.decisions and r.n_box > 0


def test_replay_refuses_what_breaks_the_contract():
    # the exponent D in place of D - 1
    logp, lo, hi, p0, chain, lp, acc = host_case(7, 16, 40, exponent=7)
    with pytest.raises(AssertionError, match="acceptance test"):
        SR.replay_chain(chain, lp, acc, p0, lo, hi, SEED, 2, lambda v: -logp(v))
    # another seed, another global problem index, a seed without its high word
    logp, lo, hi, p0, chain, lp, acc = host_case(2, 6, 40)
    for seed, gp in ((SEED + 1, 2), (SEED, 3), (SEED & 0xFFFFFFFF, 2)):
        with pytest.raises(AssertionError):
            SR.replay_chain(chain, lp, acc, p0, lo, hi, seed, gp, lambda v: -logp(v))
    # a wrong count, a log-probability that is not the likelihood's
    with pytest.raises(AssertionError, match="count of moves"):
        SR.replay_chain(chain, lp, acc + 1, p0, lo, hi, SEED, 2, lambda v: -logp(v))
    with pytest.raises(AssertionError):
        SR.replay_chain(chain, lp + 1e-13, acc, p0, lo, hi, SEED, 2, lambda v: -logp(v))
    # a box closed on its lower side: put the bound on a proposal the chain made and run the sampler again
    r = SR.replay_chain(chain, lp, acc, p0, lo, hi, SEED, 2, lambda v: -logp(v))
    s, w = [int(a[0]) for a in np.nonzero(r.moved & (np.arange(40)[:, None] < 3))]
    lo2 = lo.copy()
    lo2[0] = r.q[s, w, 0]
    good = SR.host_chain(logp, p0, lo2, hi, 40, SEED, 2)
    assert np.array_equal(good[0][:s], chain[:s]) and not np.array_equal(good[0][s, w], chain[s, w])
    SR.replay_chain(*good, p0, lo2, hi, SEED, 2, lambda v: -logp(v))
    bad = SR.host_chain(logp, p0, lo2, hi, 40, SEED, 2, strict=False)
    assert np.array_equal(bad[0][s, w], chain[s, w])
    with pytest.raises(AssertionError, match="open box"):
        SR.replay_chain(*bad, p0, lo2, hi, SEED, 2, lambda v: -logp(v))
