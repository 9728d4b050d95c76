"""Every decision of every chain against the documented random stream (include/crimp_hip.h, crimp_timing_mcmc): the
chains of crimp_timing_mcmc, crimp_orbit_mcmc and crimp_photon_mcmc replayed on the host by tests/stream_reference.py.

From a finished chain alone -- the partner as the other half stood, z and the acceptance uniform from the Philox
counter (global problem, step, walker, draw) -- the replay asserts that every move is the proposal bit for bit (in one
of the two roundings a build may give c - (c - x) z, the same one for the whole session), that nothing outside the open
box or with a non-finite log-probability was accepted, that the stored log-probability of a move is the likelihood
entry point's value there, that the device moved exactly where log u' < (D - 1) log z + lnew - lold says so (decisions
within 2^-48 max(1, |lnew|, |lold|) of equality are taken from the device, at most one per chain), and that `accepted`
counts the moves. The likelihood kernels are pinned elsewhere; here they are the means of the replay.

Every chain starts from the last step of a burn-in chain of the same entry point under another seed, and every case
has to show at least 10 % accepted and 10 % rejected decisions, so the acceptance rule is tested from both sides.

Measured on the MI355X, decisions / accepted / outside the box / non-finite / ambiguous (every chain moves by the fused
rounding):
    timing a D=1 W=2 100/90/0/0/0; D=2 W=4 200/145/2/0/0 (seed 11: 200/131/4/0/0); W=6 300/199/8/0/0;
    W=256 1536/1055/24/0/0; W=8 with a walker outside 240/175/8/0/0; the bound on a proposal 200/139/10/0/0;
    timing c D=6 360/192/0/0/0; d D=8 480/221/0/0/0; b D=9 540/167/152/0/0; gp=5 160/120/1/0/0, gp=6 160/105/8/0/0;
    orbit ell1_amxp D=7 480/210/104/0/0; bt_full D=11 660/225/177/0/0;
    photon D=2 W=4 160/115/2/0/0; W=32 1280/898/27/0/0; D=3 W=6 240/157/9/0/0.
"""
import copy

import numpy as np
import pytest

import stream_reference as SR
import test_gpu_orbit_fit as OF
import test_gpu_photon_fit as PF
import test_gpu_timing_fit as TF

pytestmark = pytest.mark.gpu

# the fixtures of the three fits' own test modules
side, nllgold, fixture, drawn = TF.side, TF.nllgold, OF.fixture, PF.drawn

SEED = 0x9E3779B97F4A7C15       # both key words non-zero and distinct
BURN_SEED = 0x0BADC0DE00000007  # the burn-in chains' seed
SESSION = {}                    # 'variant': the proposal's rounding the first chain showed; every later one must agree


def report(label, r):
    print("%-34s decisions %5d accepted %5d box %4d non-finite %4d ambiguous %d rounding %s"
          % (label, r.decisions, r.n_accepted, r.n_box, r.n_nonfinite, r.n_ambiguous, "/".join(r.found)))


def replay(label, out, p0, lo, hi, seed, gp, nll, want_box=False):
    """Replay one chain, print its row and hold it to the shares of accepted and rejected decisions."""
    chain, logprob, accepted = out
    r = SR.replay_chain(chain, logprob, accepted, p0, lo, hi, seed, gp, nll, variant=SESSION.get("variant"))
    report(label, r)
    if r.variant is not None:
        SESSION["variant"] = r.variant
    assert r.n_ambiguous <= 1
    assert r.n_accepted >= 0.1 * r.decisions, "fewer than 10 % of the decisions accepted"
    assert r.decisions - r.n_accepted >= 0.1 * r.decisions, "fewer than 10 % of the decisions rejected"
    if want_box:
        assert r.n_box >= 1, "no proposal left the box"
    return r


# ------------------------------------------------------------------ the timing fit (k_fit_mcmc<TimingLik>)
def timing_fit(side, nllgold, case, n, keys=None):
    from crimp_amd.utilities_fittoas import DeviceFit
    g, c = nllgold[case], side["cases"][case]
    return DeviceFit(g["x_%d" % n], copy.deepcopy(c["model"]), c["keys"] if keys is None else keys, g["y_%d" % n],
                     g["e_%d" % n])


def linear_case(side, nllgold, n, D):
    """Case (a) on n ToAs with F0 (D = 1) or F0 and F1 (D = 2) free: the fit, the exact solution and its sigma."""
    g = nllgold["a"]
    x, y, e = g["x_%d" % n], g["y_%d" % n], g["e_%d" % n]
    pep = side["cases"]["a"]["model"]["PEPOCH"]["value"]
    if D == 2:
        sol, cov = TF.linear_solution(x, y, e, pep)
        return timing_fit(side, nllgold, "a", n), sol, np.sqrt(np.diag(cov))
    a = (x - pep) * 86400.0
    a, w = a - a.mean(), 1.0 / e ** 2
    var = 1.0 / np.sum(w * a * a)
    return timing_fit(side, nllgold, "a", n, ["F0"]), np.array([var * np.sum(w * a * (y - y.mean()))]), \
        np.array([np.sqrt(var)])


def timing_chain(fit, p0, lo, hi, steps, seed, first_problem=0):
    ch, lp, acc = TF.run_chain(fit, p0, lo, hi, steps, seed, first_problem)
    return ch[0], lp[0], acc[0]


def burned(run, p0, burn):
    """The last step of a burn-in chain from p0 under the burn-in seed."""
    return np.ascontiguousarray(run(p0, burn, BURN_SEED)[0][-1])


@pytest.mark.parametrize("D, n, W, steps, seed", [
    (1, 84, 2, 50, SEED),       # half = 1: the partner is always the one other walker; (D - 1) log z = 0
    (2, 84, 4, 50, SEED),       # proposals leave the box sol +- 4 sigma
    (2, 84, 4, 50, 11),         # a seed whose high word is 0
    (2, 84, 6, 50, SEED),       # half = 3 is odd
    (2, 65, 256, 6, SEED),      # 16 walkers per wave and half: the wave loop; every partner index up to 127
])
def test_timing_chain_of_the_linear_problem(gpu, side, nllgold, D, n, W, steps, seed):
    fit, sol, sig = linear_case(side, nllgold, n, D)
    lo, hi = sol - 4 * sig, sol + 4 * sig
    # D = 1 with its two walkers accepts 90 to 93 of the 100 proposals of this seed whatever the start (the host
    # sampler of stream_reference on 120 starts; 92 % inside a box of 4, 2 or 1 sigma alike): the start whose chain
    # rejects 10 is used
    rng = np.random.default_rng(5 if D == 1 else W + D)

    def run(p0, k, sd):
        return timing_chain(fit, p0, lo, hi, k, sd)
    p0 = burned(run, sol + rng.uniform(-3, 3, (W, D)) * sig, 200)
    r = replay("timing a D=%d n=%d W=%d seed=%#x" % (D, n, W, seed), run(p0, steps, seed), p0, lo, hi, seed, 0,
               fit.nll, want_box=W in (4, 6))
    if W == 256:    # every partner of both halves was drawn
        _, cw = SR.draw(seed, 0, np.arange(steps)[:, None], np.arange(W)[None, :], W // 2, np.arange(W)[None, :] % 2)
        assert np.unique(cw).size == W


def test_timing_walker_that_starts_outside_the_box(gpu, side, nllgold):
    """One walker of p0 outside the box: its log-probability is -inf until it moves, and it moves on its first
    proposal that is inside the box with a finite log-probability, whatever the uniform."""
    fit, sol, sig = linear_case(side, nllgold, 84, 2)
    lo, hi = sol - 4 * sig, sol + 4 * sig
    rng = np.random.default_rng(8)
    W, steps, out = 8, 30, 3

    def run(p0, k, sd):
        return timing_chain(fit, p0, lo, hi, k, sd)
    p0 = burned(run, sol + rng.uniform(-3, 3, (W, 2)) * sig, 200)
    p0[out] = hi + np.array([0.5, -1.0]) * sig      # past the upper bound of F0 alone
    chain, logprob, accepted = run(p0, steps, SEED)
    r = replay("timing a D=2 W=8, walker 3 outside", (chain, logprob, accepted), p0, lo, hi, SEED, 0, fit.nll,
               want_box=True)
    assert np.isneginf(r.lold[0, out])
    first = int(np.argmax(r.finite[:, out]))        # its first proposal inside the box with a finite value
    assert r.finite[first, out] and r.moved[first, out] and not r.moved[:first, out].any()
    assert np.all(np.isneginf(logprob[:first, out])) and np.array_equal(chain[:first, out], np.tile(p0[out], (first, 1)))
    assert np.isfinite(logprob[first:, out]).all()


def test_timing_proposal_exactly_on_the_bound_is_rejected(gpu, side, nllgold):
    """The box is open: the lower bound of F0 is put on the smallest F0 the chain moved to, bit for bit, and the chain
    run again. Up to that decision nothing changes; there the device has to reject."""
    fit, sol, sig = linear_case(side, nllgold, 84, 2)
    lo, hi = sol - 4 * sig, sol + 4 * sig
    rng = np.random.default_rng(6)
    W, steps = 4, 50

    def run(p0, k, sd, lo=lo):
        return timing_chain(fit, p0, lo, hi, k, sd)
    p0 = burned(run, sol + rng.uniform(-3, 3, (W, 2)) * sig, 200)
    first = run(p0, steps, SEED)
    r = replay("timing a D=2 W=4 (before the bound)", first, p0, lo, hi, SEED, 0, fit.nll, want_box=True)
    q0 = np.where(r.moved, r.q[:, :, 0], np.inf)
    s, w = np.unravel_index(int(np.argmin(q0)), q0.shape)
    assert q0[s, w] < p0[:, 0].min() and np.sum(r.q[:, :, 0] == q0[s, w]) == 1
    lo2 = lo.copy()
    lo2[0] = q0[s, w]
    again = run(p0, steps, SEED, lo=lo2)
    r2 = replay("timing a D=2 W=4 (bound on a proposal)", again, p0, lo2, hi, SEED, 0, fit.nll, want_box=True)
    assert r2.q[s, w, 0] == lo2[0] and not r2.inbox[s, w] and not r2.moved[s, w]
    assert np.array_equal(again[0][:s], first[0][:s]) and np.array_equal(again[0][s, :w], first[0][s, :w])
    assert np.array_equal(again[0][s, w], (p0 if s == 0 else first[0][s - 1])[w])


HIGH_D = {  # case -> (burn-in steps, start and box of its keys as (centre, scatter, lo, hi); None: 0, tiny, open)
    "c": (1500, {}),
    "d": (3000, {}),
    "b": (300, {"GLEP_1": ("mid", 1.0, "mid-5", "mid+5"), "GLTD_1": (30.0, 0.5, 28.0, 32.0)}),
}
SCALE = {"F0": 1e-10, "F1": 1e-17, "F2": 1e-24, "GLPH_1": 1e-3, "GLF0_1": 1e-10, "GLF1_1": 1e-17, "GLF0D_1": 1e-10}


@pytest.mark.parametrize("case, D", [("c", 6), ("d", 8), ("b", 9)])
def test_timing_chain_with_waves_and_a_glitch_free(gpu, side, nllgold, case, D):
    """W = 2 D walkers (lanes past D idle), the exponent (D - 1) at D > 2, the wave and glitch slots of the map. The
    data hold no glitch and no wave, so the walkers start in a small ball around 0 and the burn-in chain lets the
    ensemble grow into the posterior. Case (b)'s 65 ToAs have two gaps of ~200 d, which leave the glitch's terms
    poorly separated, and the posterior is a funnel in GLEP and GLTD that 18 walkers sample worse the longer they run
    (5.6 % accepted after 3000 steps with both free over the span, 7.2 % with them boxed as here). The box keeps GLEP within 5 d of
    the middle of the data and GLTD in (28, 32) d, and the burn-in stops at 300 steps, when the ensemble has reached
    the mode and about 30 % of its proposals are accepted."""
    fit = timing_fit(side, nllgold, case, 65)
    keys = fit.keys
    assert len(keys) == D
    burn, special = HIGH_D[case]
    W, steps = 2 * D, 30
    rng = np.random.default_rng(D)
    centre, scatter = np.zeros(D), np.array([SCALE.get(k, 1e-3) for k in keys])
    lo, hi = np.full(D, -np.inf), np.full(D, np.inf)
    x = fit.x
    mid = 0.5 * (x.min() + x.max())
    where = {"mid": mid, "mid-5": mid - 5.0, "mid+5": mid + 5.0}
    for k, (c, sc, a, b) in special.items():
        i = keys.index(k)
        centre[i], scatter[i], lo[i], hi[i] = (where.get(v, v) for v in (c, sc, a, b))

    def run(p0, k, sd):
        return timing_chain(fit, p0, lo, hi, k, sd)
    p0 = burned(run, centre + rng.normal(0, 1, (W, D)) * scatter, burn)
    replay("timing %s D=%d n=65 W=%d" % (case, D, W), run(p0, steps, SEED), p0, lo, hi, SEED, 0, fit.nll)


def test_timing_two_problems_from_first_problem_5(gpu, side, nllgold):
    """63 + 257 ToAs in one call with first_problem = 5: the chains draw the counters of global problems 5 and 6."""
    from crimp_amd import ops
    cases = [linear_case(side, nllgold, n, 2) for n in (63, 257)]
    fits = [c[0] for c in cases]
    lo = np.stack([c[1] - 4 * c[2] for c in cases])
    hi = np.stack([c[1] + 4 * c[2] for c in cases])
    rng = np.random.default_rng(5)
    W, steps = 8, 20
    off = np.array([0, 63, 63 + 257], dtype=np.int64)

    def run(p0, k, sd, first):
        return ops.timing_mcmc(np.concatenate([f.x for f in fits]), np.concatenate([f.y for f in fits]),
                               np.concatenate([f.yerr for f in fits]), [f.fit_base for f in fits],
                               [f.wave_base for f in fits], fits[0].map, p0, lo, hi, k, sd, offsets=off,
                               first_problem=first)
    start = np.stack([c[1] + rng.uniform(-3, 3, (W, 2)) * c[2] for c in cases])
    p0 = np.ascontiguousarray(run(start, 200, BURN_SEED, 0)[0][:, -1])
    chain, logprob, accepted = run(p0, steps, SEED, 5)
    for i, fit in enumerate(fits):
        replay("timing a D=2 n=%d W=8 gp=%d" % (fit.x.size, 5 + i), (chain[i], logprob[i], accepted[i]), p0[i], lo[i],
               hi[i], SEED, 5 + i, fit.nll, want_box=True)
        # and under no other global index
        prev, _, plain, fused = SR.chain_proposals(chain[i], p0[i], SEED, i)
        assert not SR.detect_variant(chain[i], prev, plain, fused)[0]


# ------------------------------------------------------------------ the orbit fit (k_fit_mcmc<OrbitLik>)
@pytest.mark.parametrize("name", ["ell1_amxp", "bt_full"])
def test_orbit_chain(gpu, fixture, name):
    """OrbitLik through the same kernel, the fixture's keys free (7 under ELL1, 11 under BT). The data are the
    'typical' vector's residuals plus noise, so the walkers start in a small ball around that vector; an inadmissible
    proposal, if one occurs, has NLL = +inf and has to replay as a rejection."""
    c = fixture[(name, 65)]
    fit = OF.problem(c)
    D = len(c.keys)
    W, steps = max(16, 2 * D), 30
    width = np.abs(c.pvec[3])
    lo, hi = -20 * width, 20 * width
    rng = np.random.default_rng(D)

    def run(p0, k, sd):
        return OF.sample(fit, p0, lo, hi, k, sd)
    p0 = burned(run, c.pvec[3] + 1e-3 * rng.normal(0, 1, (W, D)) * width, 3000)
    replay("orbit %s D=%d n=65 W=%d" % (name, D, W), run(p0, steps, SEED), p0, lo, hi, SEED, 0, fit.nll)


# ------------------------------------------------------------------ the photon fit (k_photon_step)
@pytest.mark.parametrize("W, phoff", [(4, False), (32, False), (6, True)])
def test_photon_chain(gpu, drawn, W, phoff):
    """k_photon_step makes the proposals of a half-step one launch ahead of their acceptance; the problem index of the
    counter is 0. With phoff the free phase offset is the last of D = 3 lanes."""
    from crimp_amd.fit_photons import PhotonFit
    _, _, _, head, sol, sig = drawn
    fit = head
    if phoff:
        fit = PhotonFit(head.t, copy.deepcopy(head.parfile), PF.POSTERIOR_THETA, keys=PF.POSTERIOR_KEYS, phoff=True)
        sol, sig = np.append(sol, 0.0), np.append(sig, 5e-3)     # sigma(PHOFF): a rough scale for the start alone
    D = sol.size
    assert D == (3 if phoff else 2) and fit.t.size == 3 * PF.tile() + 17
    lo, hi = sol - 4 * sig, sol + 4 * sig
    if phoff:
        lo[-1], hi[-1] = -0.5, 0.5
    rng = np.random.default_rng(W)

    def run(p0, k, sd):
        return PF.run_chain(fit, p0, lo, hi, k, sd)
    p0 = burned(run, sol + rng.uniform(-3, 3, (W, D)) * sig, 150)
    replay("photon D=%d W=%d" % (D, W), run(p0, 40, SEED), p0, lo, hi, SEED, 0, fit.nll)
