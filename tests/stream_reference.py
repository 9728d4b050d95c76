"""The library's two documented random streams, restated on the host from their documents alone.

* The ensemble samplers (include/crimp_hip.h, crimp_timing_mcmc): Philox4x32-10, key = seed, counter = (global problem
  index, step, walker, draw); draw 0 gives the stretch factor z and the partner of the other half, draw 1 the uniform
  of the acceptance test. ``draw``, ``accept_uniform`` and ``propose`` are that text; ``replay_chain`` reconstructs
  every decision of a finished chain from the chain itself.
* The event simulator (include/crimp_hip.h, crimp_sim_events): counter = (cell low, cell high, round,
  lane), words 0-1 the gap's uniform, words 2-3 the thinning uniform. ``sim_replay`` lists every candidate of every
  cell with the outcomes a conforming device may give it.

Philox4x32-10 is Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC 2011); the
known-answer vectors of tests/test_stream_reference.py are Random123's. Everything here is NumPy on uint64 / float64 or
plain Python; ``propose`` uses ``fractions.Fraction`` for the singly rounded form.
"""
from fractions import Fraction

import numpy as np

MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # the key schedule's increments (golden ratio, sqrt(3) - 1)


def philox_words(c0, c1, c2, c3, seed):
    """Philox4x32-10 of counters given as arrays (broadcast against each other): four uint64 arrays holding the
    32-bit output words."""
    u64 = np.uint64
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & u64(MASK32) for c in (c0, c1, c2, c3)))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & MASK32, seed >> 32
    for _ in range(10):
        p0 = u64(PHILOX_M0) * c0                   # 32 x 32 -> 64 bits: exact in uint64
        p1 = u64(PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> u64(32)) ^ c1 ^ u64(k0), p1 & u64(MASK32),
                          (p0 >> u64(32)) ^ c3 ^ u64(k1), p0 & u64(MASK32))
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox4x32_10(counter, seed):
    """The four output words (Python ints) of one counter block; key = (seed low 32, seed high 32)."""
    return tuple(int(w) for w in philox_words(*[np.uint64(int(c) & MASK32) for c in counter], seed))


def uniform53(a, b):
    """(((a >> 5) << 26 | (b >> 6)) + 0.5) 2^-53 in fp64: a uniform in (0, 1] (the + 0.5 of the largest integers
    rounds in fp64, so 1.0 is reached and 0.0 is not)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    k = ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def draw(seed, gp, s, w, half, h):
    """(z, partner) of walker w = 2 k + h at step s of global problem gp: counter (gp, s, w, 0), u from words 0-1,
    z = (u + 1)^2 / 2, partner = 2 floor(word 2 * half / 2^32) + (1 - h). Arrays broadcast."""
    r0, r1, r2, _ = philox_words(gp, s, w, 0, seed)
    zr = uniform53(r0, r1) + 1.0
    partner = 2 * ((r2 * np.asarray(half, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64) + (1 - np.asarray(h))
    return zr * zr * 0.5, partner


def accept_uniform(seed, gp, s, w):
    """u' of the acceptance test: counter (gp, s, w, 1), words 0-1."""
    r0, r1, _, _ = philox_words(gp, s, w, 1, seed)
    return uniform53(r0, r1)


def propose(x, c, z):
    """The two roundings of c - (c - x) z a conforming build can produce, (plain, fused), over arrays x, c [..., D] and
    z [...]: plain fp64, and the exact product of the fp64 difference with z subtracted from c and rounded once."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64)[..., None], x.shape)
    d = c - x
    plain = c - d * z
    fused = np.empty_like(plain)
    fl = fused.reshape(-1)
    for i, (ci, di, zi) in enumerate(zip(c.reshape(-1).tolist(), d.reshape(-1).tolist(), z.reshape(-1).tolist())):
        fl[i] = float(Fraction(ci) - Fraction(di) * Fraction(zi)) if np.isfinite(ci + di + zi) else np.nan
    return plain, fused


# ------------------------------------------------------------------------------------------- the sampler's replay
class ChainReplay:
    """What ``replay_chain`` found: the tallies, and [steps, W] arrays of the replayed decisions."""


def chain_proposals(chain, p0, seed, gp):
    """From a finished chain [steps, W, D]: (prev, z, q_plain, q_fused). Walker w = 2 k + h at step s starts from
    prev[s, w] (chain[s - 1, w], p0 at s = 0) and stretches towards its partner of the other half as that half stood:
    the previous step's odd walkers for h = 0, this step's even walkers for h = 1."""
    steps, W, D = chain.shape
    prev = np.concatenate([p0[None], chain[:-1]])
    s = np.arange(steps)[:, None]
    w = np.arange(W)[None, :]
    h = w % 2
    z, cw = draw(seed, gp, s, w, W // 2, h)
    assert np.all((cw >= 0) & (cw < W) & (cw % 2 == 1 - h))
    rows = np.broadcast_to(s, cw.shape)
    c = np.where((h == 0)[..., None], prev[rows, cw], chain[rows, cw])
    plain, fused = propose(prev, c, z)
    return prev, z, plain, fused


def detect_variant(chain, prev, plain, fused):
    """The roundings ('plain', 'fused') under which EVERY moved row of the chain equals its proposal bit for bit, and
    the mask of moved rows. An empty tuple: some move is neither, or the chain mixes the two."""
    moved = np.any(chain != prev, axis=2)
    ok = {"plain": np.all(chain == plain, axis=2), "fused": np.all(chain == fused, axis=2)}
    return tuple(v for v in ("plain", "fused") if np.all(ok[v][moved])), moved, ok


def replay_chain(chain, logprob, accepted, p0, lo, hi, seed, gp, nll, variant=None):
    """Every decision of one chain against the documented stream. ``nll(vectors [P, D]) -> [P]`` is the likelihood
    entry point of the same fit, called once. ``variant``: the rounding an earlier chain of the session showed (None:
    not known yet). Asserts the proposal, box, likelihood, acceptance and count rules and returns the tallies."""
    chain, logprob, p0 = (np.asarray(a, dtype=np.float64) for a in (chain, logprob, p0))
    steps, W, D = chain.shape
    prev, z, plain, fused = chain_proposals(chain, p0, seed, gp)
    found, moved, _ = detect_variant(chain, prev, plain, fused)
    assert found, "a moved row equals neither rounding of c - (c - x) z, or the chain mixes them"
    if variant is not None:
        assert variant in found, "this chain moves by %s, an earlier one by %s" % (found, variant)
    elif len(found) == 1:
        variant = found[0]
    q = fused if (variant or found[0]) == "fused" else plain
    # the box: strict on both sides
    inbox = np.all((lo < q) & (q < hi), axis=2)
    assert not np.any(moved & ~inbox), "a proposal outside the open box was accepted"
    start_in = np.all((lo < p0) & (p0 < hi), axis=1)
    # one likelihood call: the in-box proposals, then the in-box starting positions
    vec = np.concatenate([q[inbox], p0[start_in]])
    with np.errstate(invalid="ignore"):
        val = -np.asarray(nll(np.ascontiguousarray(vec)), dtype=np.float64)
    lnew = np.full((steps, W), -np.inf)
    lnew[inbox] = val[:int(inbox.sum())]
    lstart = np.full(W, -np.inf)
    lstart[start_in] = val[int(inbox.sum()):]
    lstart[~np.isfinite(lstart)] = -np.inf
    finite = inbox & np.isfinite(lnew)
    assert not np.any(moved & ~finite), "a proposal whose log-probability is not finite was accepted"
    assert np.array_equal(logprob[moved], lnew[moved]), "a stored log-probability is not the likelihood's at the move"
    lold = np.concatenate([lstart[None], logprob[:-1]])
    # rows that did not move repeat the previous row
    still = ~moved
    assert np.array_equal(logprob[still], lold[still]), "a row that did not move changed its log-probability"
    assert np.array_equal(accepted, moved.sum(axis=0)), "accepted is not the count of moves"
    # the acceptance test, in the order the header writes it: log u' < (D - 1) log z + lnew - lold
    s = np.arange(steps)[:, None]
    w = np.arange(W)[None, :]
    logu = np.log(accept_uniform(seed, gp, s, w))
    with np.errstate(invalid="ignore"):
        m = (float(D - 1) * np.log(z) + lnew - lold) - logu
    m[finite & np.isneginf(lold)] = np.inf
    big = np.maximum(1.0, np.maximum(np.abs(lnew), np.where(np.isfinite(lold), np.abs(lold), 0.0)))
    eps = 2.0 ** -48 * np.where(finite, big, 1.0)
    must, mustnt = finite & (m > eps), finite & (m < -eps)
    assert np.all(moved[must]), "a proposal the acceptance test passes was rejected"
    assert not np.any(moved[mustnt]), "a proposal the acceptance test fails was accepted"
    out = ChainReplay()
    out.variant, out.found = variant, found
    out.moved, out.inbox, out.finite, out.lold, out.q, out.z = moved, inbox, finite, lold, q, z
    out.decisions = steps * W
    out.n_accepted = int(moved.sum())
    out.n_box = int((~inbox).sum())
    out.n_nonfinite = int((inbox & ~finite).sum())
    out.n_ambiguous = int((finite & ~must & ~mustnt).sum())
    assert out.n_ambiguous <= 1, "%d decisions within the rounding of the acceptance test" % out.n_ambiguous
    return out


def host_chain(logp, p0, lo, hi, steps, seed, gp=0, exponent=None, strict=True):
    """The documented sampler on the host (plain rounding of the proposal): (chain, logprob, accepted) of one problem
    with ``logp(vectors [P, D]) -> [P]``. ``exponent`` (default D - 1) and ``strict`` exist so that the replay's tests
    can hand it a chain that breaks the contract."""
    W, D = p0.shape
    half = W // 2
    expo = float(D - 1 if exponent is None else exponent)

    def inside(v):
        return np.all((lo < v) & (v < hi)) if strict else np.all((lo <= v) & (v < hi))
    pos = np.array(p0, dtype=np.float64)
    lp = np.array([float(logp(pos[w][None])[0]) if inside(pos[w]) else -np.inf for w in range(W)])
    lp[~np.isfinite(lp)] = -np.inf
    chain, logprob, acc = np.empty((steps, W, D)), np.empty((steps, W)), np.zeros(W, dtype=np.int64)
    for s in range(steps):
        for h in (0, 1):
            new = {}
            for w in range(h, W, 2):
                z, cw = draw(seed, gp, s, w, half, h)
                z, c = float(z), pos[int(cw)]
                q = c - (c - pos[w]) * z
                if not inside(q):
                    continue
                lq = float(logp(q[None])[0])
                if np.isfinite(lq) and np.log(float(accept_uniform(seed, gp, s, w))) < expo * np.log(z) + lq - lp[w]:
                    new[w] = (q, lq)
            for w, (q, lq) in new.items():
                pos[w], lp[w] = q, lq
                acc[w] += 1
        chain[s], logprob[s] = pos, lp
    return chain, logprob, acc


# ------------------------------------------------------------------------------------------- the simulator's replay
def scan64(x):
    """The inclusive scan of 64 values in the kernel's doubling order (distance 1, 2, 4, ..., 32; every lane adds the
    value its lower neighbour held before the step)."""
    x = np.array(x, dtype=np.float64)
    d = 1
    while d < 64:
        x[d:] = x[d:] + x[:-d]
        d <<= 1
    return x


def cell_candidates(seed, cell, lam_max, cell_s, span_s):
    """(s, u) of every candidate the rounds of one cell draw, in order: seconds since mjd_start and the thinning
    uniform; the cell's end; the number of rounds. Rounds continue until the running time passes the cell's end."""
    start = float(cell) * cell_s
    end = min(float(cell + 1) * cell_s, span_s)
    lanes = np.arange(64, dtype=np.uint64)
    base, rnd, ss, uu = 0.0, 0, [], []
    while True:
        r0, r1, r2, r3 = philox_words(cell & MASK32, cell >> 32, rnd, lanes, seed)
        offs = base + scan64(-np.log(uniform53(r0, r1)) / lam_max)
        ss.append(start + offs)
        uu.append(uniform53(r2, r3))
        base = offs[63]
        rnd += 1
        if not (start + base < end):
            break
    return np.concatenate(ss), np.concatenate(uu), end, rnd


def _ulp(x):
    return float(np.spacing(np.abs(np.float64(x))))


def sim_tolerances(mjd_start, span_s, cell_s, out_offset_s=0.0):
    """(seconds, days): how far a conforming device's candidate time may lie from the replay's. The two sides differ in
    the `log` of every gap (<= 1 ulp each side) and in whether the gap is divided by lam_max or multiplied by its
    reciprocal (1 ulp): <= 3 * 2^-52 of every gap, and a cell's gaps sum to cell_s, which with the scan's own roundings
    of those differences stays below 2^-48 cell_s. The sum with the cell's start and with the output's offset (or
    the division by 86400 and the sum with mjd_start) can then each round the other way: 2 ulp of the largest output."""
    tol_s = 2.0 ** -48 * cell_s + 2.0 * _ulp(out_offset_s + span_s)
    tol_d = 2.0 ** -48 * cell_s / 86400.0 + 2.0 * _ulp(mjd_start + span_s / 86400.0)
    return tol_s, tol_d


def _in_gti(mjd, g):
    i = np.searchsorted(g[:, 0], mjd, side="right") - 1
    return (i >= 0) & (mjd < g[np.maximum(i, 0), 1])


def sim_replay(seed, steps, bkg, lam_max, mjd_start, span_s, cell_s, cells, gti=None, frac_phase=None,
               out_offset_s=0.0):
    """Every candidate of ``cells`` from the documented stream. Returns a dict of arrays over the candidates in order:
    ``s`` (seconds since mjd_start), ``mjd``, ``outcomes`` (a list of sets over {None, 0, 1}: no event, a source
    event, a background event -- more than one entry for an ambiguous candidate) and the counts ``candidates``,
    ``ambiguous``, ``rounds`` (the largest number of rounds of a cell). ``steps``: the rate table; ``frac_phase(mjd)``
    -> the reference phases' fractional parts as floats (needed for a table of more than one rate)."""
    steps = np.asarray(steps, dtype=np.float64)
    n = steps.size
    tol_s, tol_d = sim_tolerances(mjd_start, span_s, cell_s, out_offset_s)
    g = None if gti is None else np.asarray(gti, dtype=np.float64).reshape(-1, 2)
    S_all, M_all, O_all, rounds = [], [], [], 0
    for cell in cells:
        s, u, end, r = cell_candidates(seed, int(cell), lam_max, cell_s, span_s)
        rounds = max(rounds, r)
        mjd = mjd_start + s / 86400.0
        v = u * lam_max
        alive = s < end
        alive_amb = np.abs(s - end) <= tol_s
        if g is not None:
            ing = _in_gti(mjd, g)
            gti_amb = np.min(np.abs(mjd[:, None] - g.reshape(-1)[None, :]), axis=1) <= tol_d
        else:
            ing, gti_amb = np.ones(s.size, dtype=bool), np.zeros(s.size, dtype=bool)
        live = (alive | alive_amb) & (ing | gti_amb)
        if n > 1:
            fr = np.zeros(s.size)
            fr[live] = frac_phase(mjd[live])
            pos = fr * n
            k = np.minimum(pos.astype(np.int64), n - 1)
            near = np.rint(pos)                                         # the nearest bin edge, 0 and n the same edge
            bin_amb = live & (np.abs(pos - near) / n <= 1e-9)           # 1e-9 cycles: the calcphase bound
            k2 = np.where(near > k, (k + 1) % n, (k - 1) % n)           # the bin on the other side of that edge
        else:
            k = k2 = np.zeros(s.size, dtype=np.int64)
            bin_amb = np.zeros(s.size, dtype=bool)

        def outcome(S):
            return np.where(v < S + bkg, np.where(v < S, 0, 1), -1)     # -1: thinned away
        o1, o2 = outcome(steps[k]), outcome(steps[k2])
        for i in range(s.size):
            if not live[i]:
                O_all.append({None})
                continue
            outs = {int(o1[i])} | ({int(o2[i])} if bin_amb[i] else set())
            outs = {None if o < 0 else o for o in outs}
            if alive_amb[i] or gti_amb[i] or not (alive[i] and ing[i]):
                outs.add(None)
            O_all.append(outs)
        S_all.append(s)
        M_all.append(mjd)
    return {"s": np.concatenate(S_all), "mjd": np.concatenate(M_all), "outcomes": O_all,
            "candidates": len(O_all), "ambiguous": sum(1 for o in O_all if len(o) > 1), "rounds": rounds,
            "tol_s": tol_s, "tol_d": tol_d}


def sim_match(rep, t_dev, flag_dev, days=False, out_offset_s=0.0):
    """Hold the device's event list to the replay: count, order and flags equal, times within the tolerance. Returns
    (events, ambiguous candidates met, largest |dt| / tolerance)."""
    t_host = rep["mjd"] if days else out_offset_s + rep["s"]
    tol = rep["tol_d"] if days else rep["tol_s"]
    j, worst, amb = 0, 0.0, 0
    nd = len(t_dev)
    for i, outs in enumerate(rep["outcomes"]):
        events = outs - {None}
        if not events:
            continue
        here = j < nd and abs(float(t_dev[j]) - float(t_host[i])) <= tol
        if None in outs:                       # ambiguous between an event and none: the device decides
            amb += 1
            if not here:
                continue
        elif len(outs) > 1:
            amb += 1
        assert j < nd, "the device stops after %d events; the replay has a further one at %r" % (nd, t_host[i])
        assert here, "event %d: device time %r, replay %r (tolerance %.3g)" % (j, float(t_dev[j]), float(t_host[i]),
                                                                              tol)
        assert int(flag_dev[j]) in events, "event %d at %r: background flag %d, replay %s" % (
            j, float(t_dev[j]), int(flag_dev[j]), sorted(events))
        worst = max(worst, abs(float(t_dev[j]) - float(t_host[i])) / tol)
        j += 1
    assert j == nd, "the device has %d events, the replay accounts for %d" % (nd, j)
    return j, amb, worst
