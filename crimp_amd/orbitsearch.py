"""``OrbitSearch``: the Z^2_m / H periodicity search over a grid of binary orbits (BT, ELL1), fused on the MI355X.

Not in the reference, whose PeriodSearch knows no orbit; the definition is DESIGN.md section 5.10. For every orbit of
the grid the photons' arrival times (MJD, barycentric) are taken to their emission times under that orbit and folded at
every trial frequency in one kernel (crimp_orbit_search, csrc/orbit_search.h): the first step on a pulsar whose orbit is
unknown, or known to a few percent in TASC / A1 / PB, before ``fitorbit`` has ToAs to work with.

    s = OrbitSearch(time_mjd, "pulsar.par", freq, nbrHarm=2)
    z = s.ztest(orbits, ["TASC", "A1"])                       # (norb, nf) powers; orbits holds absolute values
    pw, best = s.grid("z2", TASC=np.linspace(..), A1=np.linspace(..))
                                                              # pw (len(TASC), len(A1), nf); best: TASC, A1, Freq, Power

The spin keys of the model (F0.., glitches, waves, PEPOCH) are not used: the trial frequencies are the spin. ``tref``
(default ``(time[0] + time[-1]) / 2``, PeriodSearch's convention) is one reference epoch for all orbits, so frequencies
are comparable across the grid. There is no NumPy fallback.
"""
import argparse

import numpy as np

from . import _native as N
from . import binarymodels, ops
from ._native import STAT_H, STAT_Z2, _is_torch

_STATS = {"z2": STAT_Z2, "z": STAT_Z2, "ztest": STAT_Z2, STAT_Z2: STAT_Z2, "h": STAT_H, "htest": STAT_H}
_TINY = ("PBDOT", "A1DOT")


def product_grid(axes):
    """(keys, orbits): the product grid of ``axes`` (an ordered mapping key -> 1-D values), the first axis outermost;
    orbits has one row per orbit and one column per key."""
    keys = list(axes)
    vals = [np.atleast_1d(np.asarray(axes[k], dtype=np.float64)).ravel() for k in keys]
    if not keys:
        return keys, np.zeros((1, 0))
    mesh = np.meshgrid(*vals, indexing="ij")
    return keys, np.stack([g.ravel() for g in mesh], axis=1)


def check_orbits(base, keys, orbits):
    """ValueError naming the first orbit of ``orbits`` [norb, nkeys] outside the limits of crimp_binary_delay
    (``binarymodels.binary_params``: PB > 0, A1 >= 0, ECC in [0, 1) or EPS1^2 + EPS2^2 < 1, 2 pi A1 / (PB (1 - e)) <
    1/2), or for a key the model's kind does not have. ``base``: the plain model dict. Needs no GPU."""
    p = binarymodels.binary_params(base)
    if p is None:
        raise ValueError("the timing model has no BINARY")
    idx = ops.orbit_keys(keys, p["kind"])
    bt = p["kind"] == N.BINARY_BT
    orbits = np.asarray(orbits, dtype=np.float64).reshape(-1, len(idx))
    field = {"PB": "pb", "A1": "a1", "T0": "t0", "ECC": "ecc", "OM": "om", "OMDOT": "omdot", "GAMMA": "gamma",
             "EPS1": "eps1", "EPS2": "eps2", "PBDOT": "pbdot", "A1DOT": "a1dot"}
    cols = {field[N.ORBIT_FIELDS[i]]: orbits[:, q] for q, i in enumerate(idx)}
    v = {k: cols.get(k, np.full(orbits.shape[0], float(p[k]))) for k in field.values()}
    with np.errstate(all="ignore"):
        e = v["ecc"] if bt else np.hypot(v["eps1"], v["eps2"])
        checks = (("a binary parameter is not finite", ~np.all([np.isfinite(a) for a in v.values()], axis=0)),
                  ("PB must be positive", ~(v["pb"] > 0)),
                  ("A1 must be >= 0", ~(v["a1"] >= 0)),
                  ("ECC must be in [0, 1)" if bt else "EPS1^2 + EPS2^2 must be below 1",
                   ~((e >= 0) & (e < 1)) if bt else ~(e < 1)),
                  ("2 pi A1 / (PB (1 - e)) must be below 1/2",
                   ~(2.0 * 3.141592653589793 * v["a1"] / (v["pb"] * 86400.0 * (1.0 - e)) < 0.5)))
    bad = np.full(orbits.shape[0], -1)
    for c, (_, mask) in reversed(list(enumerate(checks))):
        bad = np.where(mask, c, bad)
    hit = np.flatnonzero(bad >= 0)
    if hit.size:
        o = int(hit[0])
        raise ValueError("orbit %d (%s): %s" % (o, ", ".join("%s=%.17g" % kv for kv in zip(keys, orbits[o])),
                                                checks[int(bad[o])][0]))
    return idx, orbits


class OrbitSearch:
    """``time_mjd``: barycentric arrival times (MJD; a NumPy array, or a torch CUDA tensor, whose results stay on the
    device). ``timMod``: a .par path or a timing-model dict with a BINARY block (BT or ELL1). ``freq``: the trial
    frequencies (Hz, any grid). ``fdot`` (Hz/s, signed) is one value for the whole search."""

    def __init__(self, time_mjd, timMod, freq, nbrHarm: int = 2, fdot: float = 0.0, tref=None):
        self.time = time_mjd
        self.model = binarymodels._plain(timMod)
        if binarymodels.binary_params(self.model) is None:
            raise ValueError("the timing model has no BINARY")
        self.freq = np.ascontiguousarray(np.atleast_1d(np.asarray(
            freq.cpu().numpy() if _is_torch(freq) else freq, dtype=np.float64)).ravel())
        self.nbrHarm = int(nbrHarm)
        self.fdot = float(fdot)
        if tref is None:
            flat = time_mjd.reshape(-1) if _is_torch(time_mjd) else np.ravel(time_mjd)
            tref = float((flat[0] + flat[-1]).item()) / 2 if _is_torch(time_mjd) else (flat[0] + flat[-1]) / 2
        self.tref = float(tref)

    def _time(self):
        if _is_torch(self.time):
            import torch
            return self.time.reshape(-1).to(torch.float64).contiguous()
        return np.ascontiguousarray(np.ravel(self.time), dtype=np.float64)

    def _run(self, stat, orbits, keys, best_only=False, want_best=False):
        if self.nbrHarm < 1:
            raise ValueError("nbrHarm must be >= 1")
        keys = list(keys)
        idx, orbits = check_orbits(self.model, keys, orbits)
        orbits = orbits.copy()
        for q, k in enumerate(idx):  # the .par's 1e-12 convention of PBDOT and A1DOT
            if N.ORBIT_FIELDS[k] in _TINY:
                orbits[:, q] = [binarymodels._tiny_units(v) for v in orbits[:, q]]
        return ops.orbit_search(self._time(), self.model, idx, orbits, self.freq, self.nbrHarm, stat, fdot=self.fdot,
                                tref=self.tref, want_power=not best_only, want_best=want_best or best_only)

    def ztest(self, orbits, keys):
        """Z^2_m power of every (orbit, frequency): (norb, nf)."""
        return self._run(STAT_Z2, orbits, keys)[0]

    def htest(self, orbits, keys):
        """H power of every (orbit, frequency): (norb, nf)."""
        return self._run(STAT_H, orbits, keys)[0]

    def best(self, stat, orbits, keys):
        """(norb, 2): every orbit's largest power and its trial index, np.argmax semantics, without the power array."""
        return self._run(_STATS[stat], orbits, keys, best_only=True)[1]

    def grid(self, stat, best_only=False, **axes):
        """The product grid of ``axes`` (e.g. ``TASC=np.linspace(..), A1=np.linspace(..)``), the first axis outermost:
        (powers reshaped to (len(ax1), ..., nf), DataFrame of the per-orbit bests with columns: the axes, Freq, Power).
        ``best_only=True`` skips the power array (None is returned in its place)."""
        import pandas as pd
        if stat not in _STATS:
            raise ValueError("stat must be 'z2' or 'h'")
        keys, orbits = product_grid(axes)
        pw, best = self._run(_STATS[stat], orbits, keys, best_only=best_only, want_best=True)
        b = best.cpu().numpy() if _is_torch(best) else np.asarray(best)
        cols = {k: orbits[:, q] for q, k in enumerate(keys)}
        if b.shape[0]:
            cols["Freq"] = self.freq[b[:, 1].astype(np.int64)]
            cols["Power"] = b[:, 0]
        else:  # no orbit or no trial frequency
            cols["Freq"] = cols["Power"] = np.full(orbits.shape[0], np.nan)
        if pw is not None:
            pw = pw.reshape(tuple(np.size(axes[k]) for k in keys) + (self.freq.size,))
        return pw, pd.DataFrame(cols)


# ------------------------------------------------------------------------------------------------------------ CLI
def _parse_axis(text):
    """KEY=lo:hi:n -> (KEY, np.linspace(lo, hi, n))."""
    key, _, spec = text.partition("=")
    parts = spec.split(":")
    if not key or len(parts) != 3:
        raise argparse.ArgumentTypeError("an axis is KEY=lo:hi:n, got %r" % text)
    return key.strip().upper(), np.linspace(float(parts[0]), float(parts[1]), int(parts[2]))


def load_axes(axes_yaml, axis_flags):
    """The ordered axes of the search: a YAML mapping KEY: {min, max, n} (or KEY: [values]) first, then every
    ``-a KEY=lo:hi:n`` flag."""
    axes = {}
    if axes_yaml:
        import yaml
        with open(axes_yaml) as fh:
            for k, v in (yaml.safe_load(fh) or {}).items():
                axes[str(k).upper()] = (np.linspace(float(v["min"]), float(v["max"]), int(v["n"]))
                                        if isinstance(v, dict) else np.asarray(v, dtype=np.float64))
    for k, v in axis_flags or []:
        axes[k] = v
    return axes


def load_times(path, ene_low=None, ene_high=None):
    """Arrival times (MJD) of a .npy array or of a barycentred event file."""
    if str(path).endswith(".npy"):
        return np.load(path, allow_pickle=False).astype(np.float64).ravel()
    from .eventfile import EvtFileOps
    ef = EvtFileOps(path).build_time_energy_df()
    if ene_low is not None or ene_high is not None:
        ef = ef.filtenergy(eneLow=0.0 if ene_low is None else ene_low, eneHigh=np.inf if ene_high is None else ene_high)
    return ef.time_energy_df["TIME"].to_numpy(dtype=float)


def build_parser():
    p = argparse.ArgumentParser(description="Z^2 / H search over a grid of binary orbits (BT, ELL1) around a "
                                            "frequency window")
    p.add_argument("events", help="barycentred event file, or a .npy array of arrival times (MJD)", type=str)
    p.add_argument("parfile", help=".par file with the BINARY block the grid is built around", type=str)
    p.add_argument("outfile", help="text table of the best trial per orbit", type=str)
    p.add_argument("-ay", "--axes_yaml", type=str, default=None, help="YAML: KEY: {min, max, n} per orbit axis")
    p.add_argument("-a", "--axis", type=_parse_axis, action="append", default=[],
                   help="an orbit axis KEY=lo:hi:n (repeatable; the first axis is the outermost)")
    p.add_argument("-fl", "--freq_low", type=float, required=True, help="lowest trial frequency (Hz)")
    p.add_argument("-fh", "--freq_high", type=float, required=True, help="highest trial frequency (Hz)")
    p.add_argument("-nf", "--nbr_freq", type=int, default=16, help="number of trial frequencies (default = 16)")
    p.add_argument("-fd", "--fdot", type=float, default=0.0, help="frequency derivative (Hz/s, default = 0; a negative value in scientific notation as -fd=-3e-11)")
    p.add_argument("-nh", "--nbrHarm", type=int, default=2, help="number of harmonics (default = 2)")
    p.add_argument("-s", "--stat", choices=["z2", "h"], default="z2", help="statistic (default = z2)")
    p.add_argument("-el", "--eneLow", type=float, default=None, help="low energy cut of an event file (keV)")
    p.add_argument("-eh", "--eneHigh", type=float, default=None, help="high energy cut of an event file (keV)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    axes = load_axes(args.axes_yaml, args.axis)
    if not axes:
        parser.error("no orbit axis: give -ay (or --axes_yaml) or -a KEY=lo:hi:n")
    t = load_times(args.events, args.eneLow, args.eneHigh)
    if t.size == 0:
        parser.error("no photons")
    freq = np.linspace(args.freq_low, args.freq_high, args.nbr_freq)
    search = OrbitSearch(t, args.parfile, freq, nbrHarm=args.nbrHarm, fdot=args.fdot)
    _, best = search.grid(args.stat, best_only=True, **axes)
    with open(args.outfile, "w") as fh:
        fh.write("# tref %.17g  nbrHarm %d  stat %s  fdot %.17g\n" % (search.tref, args.nbrHarm, args.stat, args.fdot))
        fh.write(best.to_string(index=False, float_format=lambda v: "%.17g" % v) + "\n")
    top = best.iloc[int(np.argmax(best["Power"].to_numpy()))]
    print("Best orbit of %d:" % len(best))
    for k in best.columns:
        print("  %s: %.15g" % (k, top[k]))
    print("Wrote the best trial per orbit to %s" % args.outfile)
    return best


if __name__ == "__main__":
    main()
