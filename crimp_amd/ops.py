"""Thin typed wrappers over the C-ABI (one per entry point of include/crimp_hip.h).

Arrays are NumPy (host; staged by the library, synchronous) or torch CUDA tensors
(device; enqueued on torch's current stream). Outputs are allocated here when not
given. These are the only functions that touch the native library.
"""
import ctypes
import os

import numpy as np

from . import _native as N
from . import binarymodels


def _modeltm(tm):
    """Pack a timing-model dict (values or {value, flag}) into crimp_timing_model."""
    def val(x):
        if isinstance(x, dict) and "value" in x and "flag" in x:  # readtimingmodel.py:309-321
            return x["value"]
        return x
    d = {k: val(v) for k, v in tm.items()}
    m = N.TimingModel()
    m.pepoch = float(d["PEPOCH"])
    for i in range(13):
        m.f[i] = float(d.get("F%d" % i, 0.0))
    ngl = sum(1 for k in d if k.startswith("GLEP_"))  # calcphase.py:94
    if ngl > N.MAX_GLITCH:
        raise ValueError("at most %d glitches supported" % N.MAX_GLITCH)
    m.n_glitch = ngl
    for j in range(1, ngl + 1):
        row = [d["GLEP_%d" % j]] + [d.get("%s_%d" % (b, j), 0.0) for b in ("GLPH", "GLF0", "GLF1", "GLF2", "GLF0D", "GLTD")]
        for c in range(7):
            m.glitch[j - 1][c] = float(row[c])
    nw = sum(1 for k in d if k.startswith("WAVE"))  # calcphase.py:135
    if nw:
        nharm = nw - 2  # calcphase.py:142 assumes WAVEEPOCH and WAVE_OM are present
        if nharm > N.MAX_WAVE:
            raise ValueError("at most %d wave harmonics supported" % N.MAX_WAVE)
        m.wave_epoch = float(d["WAVEEPOCH"])
        m.wave_om = float(d["WAVE_OM"])
        m.n_wave = max(nharm, 0)
        for j in range(1, nharm + 1):
            m.wave_ab[j - 1][0] = float(d["WAVE%d" % j]["A"])
            m.wave_ab[j - 1][1] = float(d["WAVE%d" % j]["B"])
    if "BINARY" in d:  # the orbit (ValueError outside its limits); without it the tail stays zero: no binary
        binarymodels.fill_native(m, d)
    return m


def calcphase(t_mjd, timing_model_dict, parts=7, total=None, folded=None, want_folded=True, flags=0):
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t_mjd, np.float64)
    n = int(t_mjd.numel() if N._is_torch(t_mjd) else np.size(t_mjd))
    if total is None:
        total = _empty_like_input(t_mjd, n, b)
    if folded is None and want_folded:
        folded = _empty_like_input(t_mjd, n, b)
    op = b.arg(total, np.float64, writable=True)
    fp = b.arg(folded, np.float64, writable=True) if folded is not None else None
    m = _modeltm(timing_model_dict)
    if m.binary:  # a model with an orbit: the requested parts at the emission time
        parts = int(parts) | N.PART_EMISSION
    with b.device_guard():
        N.check(L.crimp_calcphase(tp, n, ctypes.byref(m), int(parts), op, fp, b.flags(flags), b.stream()))
    return total, folded


def binary_delay(t_mjd, timing_model_dict, delay=None, t_emit=None, want_emit=False, flags=0):
    """(tau in seconds, emission MJD or None) of crimp_binary_delay for a flat array of arrival times (MJD)."""
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t_mjd, np.float64)
    n = int(t_mjd.numel() if N._is_torch(t_mjd) else np.size(t_mjd))
    if delay is None:
        delay = _empty_like_input(t_mjd, n, b)
    if t_emit is None and want_emit:
        t_emit = _empty_like_input(t_mjd, n, b)
    dp = b.arg(delay, np.float64, writable=True)
    ep = b.arg(t_emit, np.float64, writable=True) if t_emit is not None else None
    m = timing_model_dict if isinstance(timing_model_dict, N.TimingModel) else _modeltm(timing_model_dict)
    with b.device_guard():
        N.check(L.crimp_binary_delay(tp, n, ctypes.byref(m), dp, ep, b.flags(flags), b.stream()))
    return delay, t_emit


def _empty_like_input(a, n, b, dtype=np.float64):
    if b.device:
        import torch
        return torch.empty(n, dtype=torch.float64 if dtype == np.float64 else torch.int64, device=a.device)
    return np.empty(n, dtype=dtype)


def search_flags():
    """Extra search flags from the environment for unmodified callers: CRIMP_PRECISION=exact|nufft|f64, and
    CRIMP_SEARCH=mfma (fail unless a factorised kernel applies)."""
    f = 0
    prec = os.environ.get("CRIMP_PRECISION", "").lower()
    if prec == "f64":
        f |= N.FLAG_F64
    elif prec == "nufft":
        f |= N.FLAG_NUFFT
    elif prec == "exact":
        f |= N.FLAG_EXACT
    elif prec != "":
        raise ValueError("CRIMP_PRECISION must be exact, nufft or f64 (the fp32 'fast' path was retired)")
    if os.environ.get("CRIMP_SEARCH", "").lower() == "mfma":
        f |= N.FLAG_FORCE_MFMA
    return f


PRECISIONS = (None, "exact", "f64", "nufft")
_PRECISION_FLAGS = {None: 0, "nufft": N.FLAG_NUFFT, "exact": N.FLAG_EXACT, "f64": N.FLAG_F64}


def search(t, t0, freq, nharm, stat, log10_negfdot=None, first=0, count=None, out=None, flags=0, precision=None):
    """Z^2 / H over the fd-outer grid; computes flat trials [first, first+count).
    ``precision``: None or "nufft" (default: the non-uniform FFT wherever it applies -- an ascending progression of
    >= 64 trials per row segment and time-sorted photons --, otherwise the "exact" rule; every trial within 1e-6
    relative of the reference by its certificate and the fp64 fix-up), "exact" (no NUFFT: the exact-integer i8 MFMA
    kernel on progressions of >= 256 trials, fp64 otherwise; the default of rounds 1-5) or "f64" (fp64 kernel
    everywhere). A precision argument takes precedence over CRIMP_PRECISION."""
    return _search(t, t0, freq, nharm, stat, log10_negfdot, first, count, out, flags, precision, False)


def search_best(t, t0, freq, nharm, stat, log10_negfdot=None, first=0, count=None, out=None, flags=0,
                precision=None):
    """``search`` and the best trial of its powers in one call (crimp_search_best): (out, best power, index within
    the computed range), np.argmax semantics; a NUFFT search reads the best back with its fix-up count."""
    return _search(t, t0, freq, nharm, stat, log10_negfdot, first, count, out, flags, precision, True)


def _search(t, t0, freq, nharm, stat, log10_negfdot, first, count, out, flags, precision, want_best):
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s (the fp32 'fast' path was retired)" % (PRECISIONS,))
    env = search_flags()
    if precision is not None:
        env &= ~(N.FLAG_F64 | N.FLAG_NUFFT | N.FLAG_EXACT)
    flags |= _PRECISION_FLAGS[precision] | env
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t, np.float64)
    fp = b.arg(freq, np.float64)
    dp = b.arg(log10_negfdot, np.float64, allow_none=True)
    n = int(t.numel() if N._is_torch(t) else np.size(t))
    nf = int(freq.numel() if N._is_torch(freq) else np.size(freq))
    nfd = 0 if log10_negfdot is None else int(log10_negfdot.numel() if N._is_torch(log10_negfdot)
                                               else np.size(log10_negfdot))
    total = (nfd if nfd else 1) * nf
    if count is None:
        count = total - first
    if out is None:
        out = _empty_like_input(t, count, b)
    op = b.arg(out, np.float64, writable=True)
    if not want_best:
        with b.device_guard():
            N.check(L.crimp_search(tp, n, float(t0), fp, nf, dp, nfd, int(nharm), int(stat), int(first), int(count),
                                   op, b.flags(flags), b.stream()))
        return out
    res = np.zeros(2, dtype=np.float64)
    with b.device_guard():
        N.check(L.crimp_search_best(tp, n, float(t0), fp, nf, dp, nfd, int(nharm), int(stat), int(first), int(count),
                                    op, ctypes.c_void_p(res.ctypes.data), b.flags(flags), b.stream()))
    return out, float(res[0]), int(res[1])


def best(x):
    """(max, index) of a power array with np.argmax semantics (ties to the lowest index, NaN first), one small
    device reduction and one readback (crimp_best)."""
    n = int(x.numel() if N._is_torch(x) else np.size(x))
    if n == 0:
        raise ValueError("best of an empty array")
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    res = np.zeros(2, dtype=np.float64)
    with b.device_guard():
        N.check(L.crimp_best(xp, n, ctypes.c_void_p(res.ctypes.data), b.flags(), b.stream()))
    return float(res[0]), int(res[1])


def search_sets(t, offsets, freq, nharm, stat, flags=0):
    """One-trial Z^2 / H of many photon sets (crimp_search_sets): set i = t[offsets[i]:offsets[i+1]] (seconds) at
    freq[i], each with its own t0 = (first + last)/2. fp64. ``flags`` N.FLAG_ASYNC (device tensors): returns with the
    kernel queued on the current stream; synchronise with it before reading the result."""
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t, np.float64)
    op = b.arg(offsets, np.int64)
    fp = b.arg(freq, np.float64)
    nset = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    out = _empty_like_input(t, nset, b)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_search_sets(tp, op, nset, fp, int(nharm), int(stat), outp, b.flags(flags), b.stream()))
    return out


def make_template(model, amps, locs, wids=None, amp_shift=1.0):
    """crimp_template from arrays (model in {'fourier','cauchy','vonmises'})."""
    from scipy.special import i0
    t = N.Template()
    t.model = N.MODEL_IDS[model]
    K = len(amps)
    if not 1 <= K <= N.MAX_COMP:
        raise ValueError("template needs 1..%d components" % N.MAX_COMP)
    t.ncomp = K
    for j in range(K):
        t.amp[j] = float(amps[j])
        t.loc[j] = float(locs[j])
        if wids is not None:
            t.wid[j] = float(wids[j])
            t.i0[j] = float(i0(1.0 / float(wids[j]) ** 2)) if model == "vonmises" else 1.0
    t.amp_shift = float(amp_shift)
    return t


def toa_points(x, offsets, tpl, pt_interval, pt_norm, pt_phi):
    """[npts, 8] sums (see crimp_toa_points) in fp64 on host."""
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    ip = b.arg(pt_interval, np.int64)
    npp = b.arg(pt_norm, np.float64)
    pp = b.arg(pt_phi, np.float64)
    npts = int(pt_norm.numel() if N._is_torch(pt_norm) else np.size(pt_norm))
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    out = _empty_like_input(x, npts * 8, b)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_points(xp, op, nint, ctypes.byref(tpl), ip, npp, pp, npts, outp, b.flags(), b.stream()))
    return out.reshape(npts, 8)


def toa_shape_points(x, offsets, tpls, pt_interval, pt_norm, pt_phi, aux=None):
    """[npts, CRIMP_SHAPE_SUMS] extended-LL sums with template-shape gradients (crimp_toa_shape_points):
    point p = interval pt_interval[p] with its own template tpls[p]; aux[p, j] = I1/I0(1/wid_j^2) for
    von Mises templates. Templates, intervals and aux are host data; pt_norm/pt_phi follow x."""
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    npts = len(tpls)
    arr = (N.Template * max(npts, 1))(*tpls)
    pint = np.ascontiguousarray(pt_interval, dtype=np.int64)
    if pint.size != npts:
        raise ValueError("one interval per point")
    if b.device:
        import torch
        pt_norm = torch.as_tensor(np.asarray(pt_norm, np.float64), device=x.device)
        pt_phi = torch.as_tensor(np.asarray(pt_phi, np.float64), device=x.device)
    npp = b.arg(pt_norm, np.float64)
    pp = b.arg(pt_phi, np.float64)
    auxa = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(npts, N.MAX_COMP)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    out = _empty_like_input(x, npts * N.SHAPE_SUMS, b)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_shape_points(xp, op, nint, arr, None if auxa is None else auxa.ctypes.data,
                                         pint.ctypes.data, npp, pp, npts, outp, b.flags(), b.stream()))
    out = out.cpu().numpy() if N._is_torch(out) else out
    return out.reshape(npts, N.SHAPE_SUMS)


def toa_grid(x, offsets, tpl, norms, phis):
    """lnsum [nint, nnorm, nphi], hmin [nint, nphi] of the brute grid (fp64 accumulation)."""
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    norms = np.asarray(norms, dtype=np.float64) if not N._is_torch(norms) else norms
    nnorm = int(norms.shape[-1])
    np_ = b.arg(norms, np.float64)
    pp = b.arg(phis, np.float64)
    nphi = int(phis.numel() if N._is_torch(phis) else np.size(phis))
    ln = _empty_like_input(x, nint * nnorm * nphi, b)
    hm = _empty_like_input(x, nint * nphi, b)
    lp = b.arg(ln, np.float64, writable=True)
    hp = b.arg(hm, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_grid(xp, op, nint, ctypes.byref(tpl), np_, nnorm, pp, nphi, lp, hp, b.flags(), b.stream()))
    return ln.reshape(nint, nnorm, nphi), hm.reshape(nint, nphi)


TOA_BRUTE, TOA_VARY_AMPS = 1, 2


def toa_fit(x, offsets, tpl, exposure, norm0, ph_shift_res=1000, brutemin=False, vary_amps=False, flags=0):
    """Whole per-interval ToA fits on the device (crimp_toa_fit): [nint, 8] = norm, phShift, LLmax,
    phShift_LL, phShift_UL, likelihood evaluations, ampShift."""
    options = (TOA_BRUTE if brutemin else 0) | (TOA_VARY_AMPS if vary_amps else 0)
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    ep = b.arg(exposure, np.float64)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    out = _empty_like_input(x, nint * 8, b)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_fit(xp, op, nint, ctypes.byref(tpl), ep, float(norm0), int(ph_shift_res), options, outp,
                                b.flags(flags), b.stream()))
    return out.reshape(nint, 8)


def toa_fit_redchi2(x, offsets, tpl, exposure, norm0, ph_shift_res, brutemin, vary_amps, edges, centers, nfree,
                    flags=0, packed=False):
    """toa_fit and toa_redchi2 in one call (crimp_toa_fit_redchi2): ([nint, 8] records, [nint] redChi2), views of
    one buffer; ``packed``: that buffer itself ([9 nint]: the records, then redChi2), for a single readback."""
    options = (TOA_BRUTE if brutemin else 0) | (TOA_VARY_AMPS if vary_amps else 0)
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    ep = b.arg(exposure, np.float64)
    eg = b.arg(edges, np.float64)
    cg = b.arg(centers, np.float64)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    nb = int((centers.numel() if N._is_torch(centers) else np.size(centers)))
    buf = _empty_like_input(x, nint * 9, b)
    out, red = buf[:nint * 8], buf[nint * 8:]
    outp = b.arg(out, np.float64, writable=True)
    redp = b.arg(red, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_fit_redchi2(xp, op, nint, ctypes.byref(tpl), ep, float(norm0), int(ph_shift_res), options,
                                        eg, cg, nb, int(nfree), outp, redp, b.flags(flags), b.stream()))
    return buf if packed else (out.reshape(nint, 8), red)


def toa_redchi2(x, offsets, tpl, exposure, records, edges, centers, nfree):
    """redChi2 of every interval from its fit record (crimp_toa_redchi2: histogram + template curve + chi2 on the
    device, measureToAs.py:385-393); ``records`` [nint, 8] as toa_fit returns them."""
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    ep = b.arg(exposure, np.float64)
    rp = b.arg(records, np.float64)
    eg = b.arg(edges, np.float64)
    cg = b.arg(centers, np.float64)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    nb = int((centers.numel() if N._is_torch(centers) else np.size(centers)))
    out = _empty_like_input(x, nint, b)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_toa_redchi2(xp, op, nint, ctypes.byref(tpl), ep, rp, eg, cg, nb, int(nfree), outp,
                                    b.flags(), b.stream()))
    return out


def binphases_counts(x, offsets, edges):
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    op = b.arg(offsets, np.int64)
    ep = b.arg(edges, np.float64)
    nint = int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1)
    nb = int((edges.numel() if N._is_torch(edges) else np.size(edges)) - 1)
    out = _empty_like_input(x, nint * nb, b, dtype=np.int64)
    cp = b.arg(out, np.int64, writable=True)
    with b.device_guard():
        N.check(L.crimp_binphases(xp, op, nint, ep, nb, cp, b.flags(), b.stream()))
    return out.reshape(nint, nb)


def phase_cube(x, model=None, y=None, y_edges=None, z=None, z_edges=None, ph_edges=None, nph=None, options=0,
               flags=0):
    """The (y, z, phase) count cube of crimp_phase_cube: int64 [ny, S], S = sum of the z columns' phase bins (column j
    is [:, zoff[j] : zoff[j + 1]], zoff the prefix sum of the bin counts), a NumPy array for host inputs and a tensor
    on the photons' GPU for device tensors.

    ``x``: folded phases, or -- with ``model`` (a timing-model dict) -- MJD times folded on the device in the same pass
    (calcphase's folded phase, exactly). ``y`` / ``z`` with ``y_edges`` / ``z_edges``: the two other axes (None: one
    bin that takes every photon); option ``N.CUBE_Y_IS_X``: y = x, given as ``y_edges`` alone. Phase axis:
    ``ph_edges`` -- one edge array, or one per z column -- or ``nph`` -- a bin count, or one per z column, over
    numpy.linspace(0, 1, n + 1). Every axis bins as np.histogramdd with explicit edges; ``options``
    N.CUBE_Y_OPEN_LAST / CUBE_Z_OPEN_LAST / CUBE_PH_OPEN_LAST drop a value equal to that axis's last edge. The edges
    are host data always."""
    L = N.load()
    b = N.Buffers()
    xp = b.arg(x, np.float64)
    n = int(x.numel() if N._is_torch(x) else np.size(x))
    yp = b.arg(y, np.float64, allow_none=True)
    zp = b.arg(z, np.float64, allow_none=True)
    for a in (y, z):
        if a is not None and int(a.numel() if N._is_torch(a) else np.size(a)) != n:
            raise ValueError("x, y and z differ in length")

    def host(e):
        return None if e is None else np.ascontiguousarray(e, dtype=np.float64).reshape(-1)
    ye, ze = host(y_edges), host(z_edges)
    ny = 1 if ye is None else ye.size - 1
    nz = 1 if ze is None else ze.size - 1
    if ph_edges is None:
        if nph is None:
            raise ValueError("phase_cube needs ph_edges or nph")
        bins = [int(nph)] * nz if np.isscalar(nph) else [int(v) for v in nph]
        cols = [np.linspace(0, 1, k + 1) for k in bins]
    elif isinstance(ph_edges, (list, tuple)) and len(ph_edges) and np.ndim(ph_edges[0]) == 1:
        cols = [host(e) for e in ph_edges]
    else:
        cols = [host(ph_edges)] * nz
    if len(cols) != nz:
        raise ValueError("one phase-edge array (or bin count) per z column: %d for %d columns" % (len(cols), nz))
    if min(c.size for c in cols) < 2 or ny < 1 or nz < 1:
        raise ValueError("an axis needs at least two edges")
    nphs = np.array([c.size - 1 for c in cols], dtype=np.int32)
    pe = np.ascontiguousarray(np.concatenate(cols))
    S = int(nphs.sum())
    out = _empty_like_input(x, ny * S, b, dtype=np.int64)
    cp = b.arg(out, np.int64, writable=True)
    m = None if model is None else ctypes.byref(_modeltm(model))

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)
    with b.device_guard():
        N.check(L.crimp_phase_cube(xp, n, m, yp, ptr(ye), ny, zp, ptr(ze), nz, ptr(pe), ptr(nphs), cp, int(options),
                                   b.flags(flags), b.stream()))
    return out.reshape(ny, S)


_GLITCH_FIELDS = ("GLEP", "GLPH", "GLF0", "GLF1", "GLF2", "GLF0D", "GLTD")


def fit_map(keys):
    """crimp_fit_map of a list of free-parameter names (utilities_fittoas.list_fit_keys): the model field every
    parameter overwrites and the branch of model_phase_residuals (utilities_fittoas.py:275-291) the names select."""
    import re
    if not 1 <= len(keys) <= N.FIT_MAX_DIM:
        raise ValueError("a fit needs 1..%d free parameters, got %d" % (N.FIT_MAX_DIM, len(keys)))
    m = N.FitMap()
    m.ndim = len(keys)
    m.f0_param = -1
    wave = ["wave" in k.lower() for k in keys]
    m.branch = N.FIT_WAVES_ONLY if all(wave) else N.FIT_WAVES_MIXED if any(wave) else N.FIT_WAVES_FIXED
    for i, k in enumerate(keys):
        f = re.match(r"^F(\d+)$", k)
        g = re.match(r"^(GL[A-Z0-9]+)_(\d+)$", k)
        w = re.match(r"^WAVE(\d+)_([AB])$", k)
        if f:
            slot = (N.FIT_SLOT_F, int(f.group(1)), 0)
            if slot[1] == 0:
                m.f0_param = i
        elif g and g.group(1) in _GLITCH_FIELDS:
            slot = (N.FIT_SLOT_GLITCH, int(g.group(2)) - 1, _GLITCH_FIELDS.index(g.group(1)))
        elif w:
            slot = (N.FIT_SLOT_WAVE, int(w.group(1)) - 1, "AB".index(w.group(2)))
        else:
            raise ValueError("parameter %r cannot be fitted (F0..F12, GL*_j and WAVEj_A/B can)" % k)
        m.slot[i].kind, m.slot[i].index, m.slot[i].sub = slot
    return m


def _fit_args(b, t, y, yerr, offsets, fit_bases, wave_bases, pars=None):
    """The pointers, counts and model arrays of a ToA-fit call; ``pars`` None: a binary-free fit, which refuses a base
    with an orbit."""
    if isinstance(fit_bases, N.TimingModel):
        fit_bases, wave_bases = [fit_bases], [wave_bases]
        pars = None if pars is None else [pars]
    nprob = len(fit_bases)
    if pars is None:
        if len(wave_bases) != nprob:
            raise ValueError("one fit base and one wave base per problem")
        if any(m.binary for m in fit_bases) or any(m.binary for m in wave_bases):
            raise ValueError("binary models are not fitted yet")
    elif len(pars) != nprob or len(wave_bases) != nprob:
        raise ValueError("one full model, one fit base and one wave base per problem")
    if offsets is None:
        n = int(t.numel() if N._is_torch(t) else np.size(t))
        offsets = np.array([0, n], dtype=np.int64)
        if N._is_torch(t) and t.is_cuda:
            import torch
            offsets = torch.as_tensor(offsets, device=t.device)
    if int((offsets.numel() if N._is_torch(offsets) else np.size(offsets)) - 1) != nprob:
        raise ValueError("offsets needs one entry more than there are problems")
    ptrs = (b.arg(t, np.float64), b.arg(y, np.float64), b.arg(yerr, np.float64), b.arg(offsets, np.int64), nprob)
    ntoa = int(t.numel() if N._is_torch(t) else np.size(t))
    arr = N.TimingModel * nprob
    models = (() if pars is None else (arr(*pars),)) + (arr(*fit_bases), arr(*wave_bases))
    return ptrs, nprob, ntoa, models


def _fit_nll(t, y, yerr, pars, fit_bases, wave_bases, fmap, pvec, offsets, want_mu, flags):
    L = N.load()
    b = N.Buffers()
    ptrs, nprob, ntoa, models = _fit_args(b, t, y, yerr, offsets, fit_bases, wave_bases, pars)
    nd = int(fmap.ndim)
    tot = int(pvec.numel() if N._is_torch(pvec) else np.size(pvec))
    if nd < 1 or tot == 0 or tot % (nprob * nd):
        raise ValueError("pvec must be [nprob, P, ndim]")
    P = tot // (nprob * nd)
    pp = b.arg(pvec, np.float64)
    nll = _empty_like_input(t, nprob * P, b)
    mu = _empty_like_input(t, P * ntoa, b) if want_mu else None
    nllp = b.arg(nll, np.float64, writable=True)
    mup = b.arg(mu, np.float64, writable=True) if want_mu else None
    call = L.crimp_timing_nll if pars is None else L.crimp_orbit_nll
    with b.device_guard():
        N.check(call(*ptrs, *models, ctypes.byref(fmap), pp, P, nllp, mup, b.flags(flags), b.stream()))
    nll = nll.reshape(nprob, P)
    return (nll, mu) if want_mu else nll


def _chain_outputs(b, like, nprob, steps, W, D):
    """(chain, logprob, accepted) of nprob chains, flat, placed as ``like``, and their writable pointers."""
    rows = nprob * max(steps, 0) * W
    out = (_empty_like_input(like, rows * D, b), _empty_like_input(like, rows, b),
           _empty_like_input(like, nprob * W, b, dtype=np.int64))
    return out, (b.arg(out[0], np.float64, writable=True), b.arg(out[1], np.float64, writable=True),
                 b.arg(out[2], np.int64, writable=True))


def _fit_mcmc(t, y, yerr, pars, fit_bases, wave_bases, fmap, p0, lo, hi, steps, seed, offsets, first_problem, flags):
    L = N.load()
    b = N.Buffers()
    ptrs, nprob, ntoa, models = _fit_args(b, t, y, yerr, offsets, fit_bases, wave_bases, pars)
    nd = int(fmap.ndim)
    shape = tuple(p0.shape)
    if len(shape) != 3 or shape[0] != nprob or shape[2] != nd:
        raise ValueError("p0 must be [nprob, W, ndim]")
    W, steps = int(shape[1]), int(steps)
    for a in (lo, hi):
        if int(a.numel() if N._is_torch(a) else np.size(a)) != nprob * nd:
            raise ValueError("lo and hi must be [nprob, ndim]")
    pp, lop, hip_ = b.arg(p0, np.float64), b.arg(lo, np.float64), b.arg(hi, np.float64)
    (chain, logprob, accepted), outp = _chain_outputs(b, t, nprob, steps, W, nd)
    call = L.crimp_timing_mcmc if pars is None else L.crimp_orbit_mcmc
    with b.device_guard():
        N.check(call(*ptrs, *models, ctypes.byref(fmap), pp, lop, hip_, W, steps, int(seed) & 0xFFFFFFFFFFFFFFFF,
                     int(first_problem), *outp, b.flags(flags), b.stream()))
    return chain.reshape(nprob, steps, W, nd), logprob.reshape(nprob, steps, W), accepted.reshape(nprob, W)


def timing_nll(t, y, yerr, fit_bases, wave_bases, fmap, pvec, offsets=None, want_mu=False, flags=0):
    """Gaussian NLL of the phase residuals for nprob problems x P parameter vectors in one launch (crimp_timing_nll).
    ``t, y, yerr``: the ToAs of all problems concatenated, problem i = [offsets[i], offsets[i+1]) (offsets None: one
    problem); ``fit_bases`` / ``wave_bases``: one N.TimingModel each per problem (or a single one);
    ``pvec`` [nprob, P, ndim]. Returns nll [nprob, P], or (nll, mu) with ``want_mu``: mu flat, problem i's
    mean-subtracted model residuals at mu[P * offsets[i]:] as [P, n_i]."""
    return _fit_nll(t, y, yerr, None, fit_bases, wave_bases, fmap, pvec, offsets, want_mu, flags)


def timing_mcmc(t, y, yerr, fit_bases, wave_bases, fmap, p0, lo, hi, steps, seed, offsets=None, first_problem=0,
                flags=0):
    """The ensemble sampler of nprob problems in one launch (crimp_timing_mcmc): ``p0`` [nprob, W, ndim], ``lo`` /
    ``hi`` [nprob, ndim] (+-inf: no bound). Returns (chain [nprob, steps, W, ndim], logprob [nprob, steps, W],
    accepted [nprob, W]); placement follows ``t``. Problem i draws the random stream of global index
    ``first_problem + i``."""
    return _fit_mcmc(t, y, yerr, None, fit_bases, wave_bases, fmap, p0, lo, hi, steps, seed, offsets, first_problem,
                     flags)


# names a .par gives the orbit fields under: XDOT is A1DOT, E is ECC, TASC takes T0's slot under ELL1
_ORBIT_ALIASES = {"XDOT": "A1DOT", "E": "ECC", "TASC": "T0"}


def orbit_fit_map(keys):
    """``fit_map`` for a model with an orbit: the keys ``fit_map`` knows, and the orbital keys (PB, A1, T0 | TASC, ECC
    | E, OM, OMDOT, GAMMA, EPS1, EPS2, PBDOT, A1DOT | XDOT) as FIT_SLOT_BINARY slots. The branch is chosen by the
    non-orbital keys (none: FIT_WAVES_FIXED)."""
    if not 1 <= len(keys) <= N.FIT_MAX_DIM:
        raise ValueError("a fit needs 1..%d free parameters, got %d" % (N.FIT_MAX_DIM, len(keys)))
    orbital = [_ORBIT_ALIASES.get(k, k) in N.ORBIT_FIELDS for k in keys]
    spin = [k for k, o in zip(keys, orbital) if not o]
    sm = fit_map(spin) if spin else None
    m = N.FitMap()
    m.ndim = len(keys)
    m.f0_param = -1
    m.branch = sm.branch if sm is not None else N.FIT_WAVES_FIXED
    j = 0
    for i, (k, o) in enumerate(zip(keys, orbital)):
        if o:
            m.slot[i].kind, m.slot[i].index, m.slot[i].sub = (N.FIT_SLOT_BINARY,
                                                              N.ORBIT_FIELDS.index(_ORBIT_ALIASES.get(k, k)), 0)
        else:
            m.slot[i].kind, m.slot[i].index, m.slot[i].sub = sm.slot[j].kind, sm.slot[j].index, sm.slot[j].sub
            if sm.f0_param == j:
                m.f0_param = i
            j += 1
    return m


def orbit_nll(t, y, yerr, pars, fit_bases, wave_bases, fmap, pvec, offsets=None, want_mu=False, flags=0):
    """``timing_nll`` for models with an orbit (crimp_orbit_nll): ``pars`` is the full model of every problem, with its
    binary block; ``fmap`` an ``orbit_fit_map``. A vector whose corrected orbit is outside the limits gives +inf."""
    return _fit_nll(t, y, yerr, pars, fit_bases, wave_bases, fmap, pvec, offsets, want_mu, flags)


def orbit_mcmc(t, y, yerr, pars, fit_bases, wave_bases, fmap, p0, lo, hi, steps, seed, offsets=None, first_problem=0,
               flags=0):
    """``timing_mcmc`` for models with an orbit (crimp_orbit_mcmc); the arguments of ``orbit_nll`` and ``timing_mcmc``,
    the same outputs."""
    return _fit_mcmc(t, y, yerr, pars, fit_bases, wave_bases, fmap, p0, lo, hi, steps, seed, offsets, first_problem,
                     flags)


def orbit_keys(keys, kind):
    """CRIMP_ORBIT_* indices of the orbit keys ``keys`` (PB, A1, T0 | TASC, ECC | E, OM, OMDOT, GAMMA, EPS1, EPS2,
    PBDOT, A1DOT | XDOT) for a model of ``kind`` (N.BINARY_BT | N.BINARY_ELL1). ValueError for a name that is no orbit
    key, a key named twice, or a key the kind does not have (T0, ECC, OM, OMDOT, GAMMA under ELL1; TASC, EPS1, EPS2
    under BT)."""
    keys = list(keys)
    if len(keys) > len(N.ORBIT_FIELDS):
        raise ValueError("at most %d orbit keys, got %d" % (len(N.ORBIT_FIELDS), len(keys)))
    bt = kind == N.BINARY_BT
    refused = ("TASC", "EPS1", "EPS2") if bt else ("T0", "ECC", "E", "OM", "OMDOT", "GAMMA")
    out = []
    for k in keys:
        name = _ORBIT_ALIASES.get(str(k).upper(), str(k).upper())
        if name not in N.ORBIT_FIELDS:
            raise ValueError("%r is not an orbit key (%s, TASC, E, XDOT)" % (k, ", ".join(N.ORBIT_FIELDS)))
        if str(k).upper() in refused:
            raise ValueError("%s is not a key of a %s orbit" % (k, "BT" if bt else "ELL1"))
        idx = N.ORBIT_FIELDS.index(name)
        if idx in out:
            raise ValueError("orbit key %s is named twice" % k)
        out.append(idx)
    return out


def orbit_search(t_mjd, base, keys, orbits, freq, nharm, stat, fdot=0.0, tref=None, first=0, count=None, power=None,
                 best=None, want_power=True, want_best=False, flags=0):
    """Z^2 / H over a grid of orbits (crimp_orbit_search): (power [count, nf] or None, best [count, 2] or None; best is
    [0, 2] when nf == 0).
    ``base``: the timing-model dict (or a packed N.TimingModel) with the BINARY block; ``keys``: orbit key names (or
    CRIMP_ORBIT_* indices); ``orbits`` [norb, nkeys]: absolute values in the .par's units, host memory; ``freq``: host
    memory; ``t_mjd``: a NumPy array or a torch CUDA tensor (the results then stay on its device). Orbits
    [first, first + count) are computed. ``tref`` defaults to (t[0] + t[-1]) / 2."""
    m = base if isinstance(base, N.TimingModel) else _modeltm(base)
    if m.binary == N.BINARY_NONE:
        raise ValueError("the timing model has no BINARY")
    kidx = [int(k) for k in keys] if all(isinstance(k, (int, np.integer)) for k in keys) else orbit_keys(keys, m.binary)
    orbits = np.ascontiguousarray(np.asarray(orbits, dtype=np.float64).reshape(-1, len(kidx)) if len(kidx)
                                  else np.zeros((np.shape(orbits)[0], 0)))
    freq = np.ascontiguousarray(np.atleast_1d(np.asarray(freq, dtype=np.float64)).ravel())
    norb, nf = orbits.shape[0], freq.size
    if count is None:
        count = norb - first
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t_mjd, np.float64)
    n = int(t_mjd.numel() if N._is_torch(t_mjd) else np.size(t_mjd))
    if tref is None:
        flat = t_mjd.reshape(-1)
        tref = float((flat[0] + flat[-1]).item()) / 2 if N._is_torch(t_mjd) else (flat[0] + flat[-1]) / 2
    if power is None and want_power:
        power = _empty_like_input(t_mjd, max(count, 0) * nf, b).reshape(max(count, 0), nf)
    if best is None and want_best:
        # (no trial, no best: nf == 0 gives an empty table)
        best = _empty_like_input(t_mjd, (max(count, 0) if nf else 0) * 2, b).reshape(max(count, 0) if nf else 0, 2)
    pp = b.arg(power, np.float64, writable=True) if power is not None else None
    bp = b.arg(best, np.float64, writable=True) if best is not None else None
    karr = np.asarray(kidx, dtype=np.int32)
    with b.device_guard():
        N.check(L.crimp_orbit_search(tp, n, ctypes.byref(m), float(tref), ctypes.c_void_p(karr.ctypes.data),
                                     len(kidx), ctypes.c_void_p(orbits.ctypes.data), norb,
                                     ctypes.c_void_p(freq.ctypes.data), nf, float(fdot), int(nharm), int(stat),
                                     int(first), int(count), pp, bp, b.flags(flags), b.stream()))
    return power, best


def _photon_args(b, t, x, par, phoff, orbit=False):
    n = int(t.numel() if N._is_torch(t) else np.size(t))
    if int(x.numel() if N._is_torch(x) else np.size(x)) != n:
        raise ValueError("t and x differ in length")
    m = par if isinstance(par, N.TimingModel) else _modeltm(par)
    if m.binary and not orbit:
        raise ValueError("binary models are not fitted yet")
    return b.arg(t, np.float64), b.arg(x, np.float64), n, m, 1 if phoff else 0


def photon_nll(t, x, par, fmap, tpl, norm, pvec, phoff=False, want_delta=False, flags=0):
    """Unbinned template NLL of the photons folded with ``par`` corrected by each of P vectors (crimp_photon_nll).
    ``t``: photon MJDs; ``x``: their folded phases under ``par`` (cycles); ``par``: a timing-model dict or
    N.TimingModel; ``fmap``: ``fit_map`` of the free keys; ``pvec`` [P, D], D = ndim + 1 with ``phoff`` (PHOFF last).
    Returns nll [P], or (nll, delta [P, n]) with ``want_delta``."""
    return _photon_nll(False, t, x, par, fmap, tpl, norm, pvec, phoff, want_delta, flags)


def photon_orbit_nll(t, x, par, fmap, tpl, norm, pvec, phoff=False, want_delta=False, flags=0):
    """``photon_nll`` for a model with an orbit (crimp_photon_orbit_nll): ``par`` carries its BINARY block, ``x`` is the
    folded phase at the emission time, ``fmap`` an ``orbit_fit_map``. A vector whose corrected orbit is outside the
    limits gives +inf and a delta row of +inf."""
    return _photon_nll(True, t, x, par, fmap, tpl, norm, pvec, phoff, want_delta, flags)


def _photon_nll(orbit, t, x, par, fmap, tpl, norm, pvec, phoff, want_delta, flags):
    L = N.load()
    b = N.Buffers()
    tp, xp, n, m, ph = _photon_args(b, t, x, par, phoff, orbit)
    D = int(fmap.ndim) + ph
    tot = int(pvec.numel() if N._is_torch(pvec) else np.size(pvec))
    if tot == 0 or tot % D:
        raise ValueError("pvec must be [P, %d]" % D)
    P = tot // D
    pp = b.arg(pvec, np.float64)
    nll = _empty_like_input(t, P, b)
    delta = _empty_like_input(t, P * n, b) if want_delta else None
    nllp = b.arg(nll, np.float64, writable=True)
    dp = b.arg(delta, np.float64, writable=True) if want_delta else None
    call = L.crimp_photon_orbit_nll if orbit else L.crimp_photon_nll
    with b.device_guard():
        N.check(call(tp, xp, n, ctypes.byref(m), ctypes.byref(fmap), ctypes.byref(tpl), float(norm), ph, pp, P, nllp,
                     dp, b.flags(flags), b.stream()))
    return (nll, delta.reshape(P, n)) if want_delta else nll


def photon_mcmc(t, x, par, fmap, tpl, norm, p0, lo, hi, steps, seed, phoff=False, flags=0):
    """The ensemble sampler of the photon likelihood (crimp_photon_mcmc): ``p0`` [W, D], ``lo`` / ``hi`` [D] (+-inf: no
    bound). Returns (chain [steps, W, D], logprob [steps, W], accepted [W]); placement follows ``t``."""
    return _photon_mcmc(False, t, x, par, fmap, tpl, norm, p0, lo, hi, steps, seed, phoff, flags)


def photon_orbit_mcmc(t, x, par, fmap, tpl, norm, p0, lo, hi, steps, seed, phoff=False, flags=0):
    """``photon_mcmc`` for a model with an orbit (crimp_photon_orbit_mcmc); the arguments of ``photon_orbit_nll`` and
    ``photon_mcmc``, the same outputs. No vector outside the orbit's limits enters the chain."""
    return _photon_mcmc(True, t, x, par, fmap, tpl, norm, p0, lo, hi, steps, seed, phoff, flags)


def _photon_mcmc(orbit, t, x, par, fmap, tpl, norm, p0, lo, hi, steps, seed, phoff, flags):
    L = N.load()
    b = N.Buffers()
    tp, xp, n, m, ph = _photon_args(b, t, x, par, phoff, orbit)
    D = int(fmap.ndim) + ph
    shape = tuple(p0.shape)
    if len(shape) != 2 or shape[1] != D:
        raise ValueError("p0 must be [W, %d]" % D)
    W, steps = int(shape[0]), int(steps)
    for a in (lo, hi):
        if int(a.numel() if N._is_torch(a) else np.size(a)) != D:
            raise ValueError("lo and hi must be [%d]" % D)
    pp, lop, hip_ = b.arg(p0, np.float64), b.arg(lo, np.float64), b.arg(hi, np.float64)
    (chain, logprob, accepted), outp = _chain_outputs(b, t, 1, steps, W, D)
    call = L.crimp_photon_orbit_mcmc if orbit else L.crimp_photon_mcmc
    with b.device_guard():
        N.check(call(tp, xp, n, ctypes.byref(m), ctypes.byref(fmap), ctypes.byref(tpl), float(norm), ph, pp, lop, hip_,
                     W, steps, int(seed) & 0xFFFFFFFFFFFFFFFF, *outp, b.flags(flags), b.stream()))
    return chain.reshape(steps, W, D), logprob.reshape(steps, W), accepted


def is_sorted(t):
    """True when the times are non-decreasing (crimp_is_sorted; a NaN counts as out of order), as
    np.all(t[1:] >= t[:-1])."""
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t, np.float64)
    n = int(t.numel() if N._is_torch(t) else np.size(t))
    flag = ctypes.c_int32(0)
    with b.device_guard():
        N.check(L.crimp_is_sorted(tp, n, ctypes.byref(flag), b.flags(), b.stream()))
    return flag.value == 0


def select_intervals(t, starts, ends):
    """(lo, count, first, last) per interval on time-sorted photons t (crimp_select_intervals): the photons
    t[lo : lo + count] are those of the reference's mask (t >= start) & (t <= end) (measureToAs.py:173-174), first /
    last their first and last time (NaN for an empty interval). Host NumPy arrays out; t stays where it is (a device
    tensor is searched on the device, the bounds go up with it)."""
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t, np.float64)
    n = int(t.numel() if N._is_torch(t) else np.size(t))
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1)
    ends = np.ascontiguousarray(ends, dtype=np.float64).reshape(-1)
    if starts.size != ends.size:
        raise ValueError("starts and ends differ in length")
    nint = int(starts.size)
    if b.device:
        import torch
        sd = torch.as_tensor(starts, device=t.device)
        ed = torch.as_tensor(ends, device=t.device)
        outi = torch.empty(2 * nint, dtype=torch.int64, device=t.device)
        outf = torch.empty(2 * nint, dtype=torch.float64, device=t.device)
        args = (b.arg(sd, np.float64), b.arg(ed, np.float64), b.arg(outi[:nint], np.int64, writable=True),
                b.arg(outi[nint:], np.int64, writable=True), b.arg(outf, np.float64, writable=True))
    else:
        outi = np.empty(2 * nint, dtype=np.int64)
        outf = np.empty(2 * nint, dtype=np.float64)
        args = (b.arg(starts, np.float64), b.arg(ends, np.float64), ctypes.c_void_p(outi.ctypes.data),
                ctypes.c_void_p(outi[nint:].ctypes.data), ctypes.c_void_p(outf.ctypes.data))
    with b.device_guard():
        N.check(L.crimp_select_intervals(tp, n, args[0], args[1], nint, args[2], args[3], args[4], b.flags(),
                                         b.stream()))
    if N._is_torch(outi):
        outi, outf = outi.cpu().numpy(), outf.cpu().numpy()
    return outi[:nint].copy(), outi[nint:].copy(), outf[0::2].copy(), outf[1::2].copy()


def gather_ranges(t, lo, offsets):
    """The photons t[lo[i] : lo[i] + (offsets[i+1] - offsets[i])] of every interval, concatenated (crimp_gather_ranges);
    same placement as t (a device tensor in, a device tensor out)."""
    L = N.load()
    b = N.Buffers()
    tp = b.arg(t, np.float64)
    n = int(t.numel() if N._is_torch(t) else np.size(t))
    lo = np.ascontiguousarray(lo, dtype=np.int64).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    nint = int(lo.size)
    if offsets.size != nint + 1:
        raise ValueError("offsets needs one entry more than lo")
    total = int(offsets[-1]) if nint else 0
    out = _empty_like_input(t, total, b)
    if b.device:
        import torch
        lp = b.arg(torch.as_tensor(lo, device=t.device), np.int64)
        op = b.arg(torch.as_tensor(offsets, device=t.device), np.int64)
    else:
        lp, op = b.arg(lo, np.int64), b.arg(offsets, np.int64)
    outp = b.arg(out, np.float64, writable=True)
    with b.device_guard():
        N.check(L.crimp_gather_ranges(tp, n, lp, op, nint, outp, b.flags(), b.stream()))
    return out


def make_sim_shape(template=None, norm=0.0, ph_shift=0.0, steps=None, bkg=0.0, lam_max=None):
    """crimp_sim_shape of the event simulator: a template shape (``template`` a crimp_template from make_template,
    with ``norm`` in counts/s and ``ph_shift`` in rad) or a step shape (``steps``: one rate per phase bin), a flat
    background ``bkg`` and the caller's rate bound ``lam_max`` >= shape + bkg at every phase."""
    if (template is None) == (steps is None):
        raise ValueError("a simulated shape is either a template or a table of steps")
    if lam_max is None:
        raise ValueError("lam_max (a bound of the rate) is required")
    sh = N.SimShape()
    if template is not None:
        sh.kind = N.SIM_TEMPLATE
        sh.tpl = template
        sh.norm, sh.ph_shift = float(norm), float(ph_shift)
        sh._steps = None
    else:
        arr = np.ascontiguousarray(steps, dtype=np.float64).reshape(-1)
        sh.kind = N.SIM_STEPS
        sh.n_steps = int(arr.size)
        sh.steps = arr.ctypes.data if arr.size else None
        sh._steps = arr  # keeps the table alive
    sh.bkg, sh.lam_max = float(bkg), float(lam_max)
    return sh


def sim_events(model, shape, mjd_start, span_s, cell_s, gti=None, seed=0, first_cell=0, n_cells=-1, out_offset_s=0.0,
               days=False, want_bkg=True, device=None, count_only=False, flags=0, cap=None):
    """Simulated events of crimp_sim_events: (time, is_bgr, n). ``model``: a timing-model dict (or N.TimingModel);
    ``shape``: make_sim_shape's; ``gti`` [ngti, 2] MJD or None. The count pass sizes the buffers, the fill pass writes
    them: NumPy arrays, or tensors on ``device`` (True: the current GPU) -- then nothing but the count crosses to the
    host. ``time`` is ``out_offset_s`` + seconds since ``mjd_start``, or MJD with ``days``; ``is_bgr`` uint8 (None
    without ``want_bkg``); ``count_only``: (None, None, n). ``cap``: the caller's estimate of the number of events --
    buffers of that size are tried first, so that a sufficient estimate saves the separate count call (the outputs are
    then views of the larger buffers)."""
    L = N.load()
    m = model if isinstance(model, N.TimingModel) else _modeltm(model)
    g = None if gti is None else np.ascontiguousarray(gti, dtype=np.float64).reshape(-1, 2)
    ngti = 0 if g is None else int(g.shape[0])
    fl = int(flags) | (N.FLAG_TIME_DAYS if days else 0)
    sh = N.SimShape.from_buffer_copy(shape)
    steps = getattr(shape, "_steps", None)
    keep = [steps, g]
    stream = None
    guard = None
    if device is not None and device is not False:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is True else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        fl |= N.FLAG_DEVICE_PTRS
        guard = torch.cuda.device(dev)
        if steps is not None and steps.size:
            sd = torch.as_tensor(steps, device=dev)
            keep.append(sd)
            sh.steps = sd.data_ptr()
        gd = torch.as_tensor(g, device=dev) if ngti else None
        keep.append(gd)
        gp = ctypes.c_void_p(gd.data_ptr()) if ngti else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    else:
        dev = None
        gp = ctypes.c_void_p(g.ctypes.data) if ngti else None
    n = ctypes.c_int64(0)

    def empty(k):
        if dev is not None:
            import torch
            return (torch.empty(k, dtype=torch.float64, device=dev),
                    torch.empty(k, dtype=torch.uint8, device=dev) if want_bkg else None)
        return np.empty(k, dtype=np.float64), (np.empty(k, dtype=np.uint8) if want_bkg else None)

    def ptr(a):
        if a is None:
            return None
        return ctypes.c_void_p(a.data_ptr() if dev is not None else a.ctypes.data)

    def call(t, b, size, may_overflow=False):
        args = (ctypes.byref(m), ctypes.byref(sh), float(mjd_start), float(span_s), float(cell_s), gp, ngti,
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_cell), int(n_cells), ptr(t), ptr(b), int(size),
                ctypes.byref(n), float(out_offset_s), fl, stream)
        if guard is not None:
            with guard:
                rc = L.crimp_sim_events(*args)
        else:
            rc = L.crimp_sim_events(*args)
        if may_overflow and rc == -1 and n.value > size:  # CRIMP_ERR_ARG: the estimate was too small
            return False
        N.check(rc)
        return True

    if g is not None and ngti == 0:  # no good time at all
        t, b = empty(0)
        return (None, None, 0) if count_only else (t, b, 0)
    if cap is not None and not count_only and int(cap) > 0:
        t, b = empty(int(cap))
        if call(t, b, int(cap), may_overflow=True):
            k = int(n.value)
            return t[:k], (None if b is None else b[:k]), k
    call(None, None, 0)
    if count_only:
        return None, None, int(n.value)
    t, b = empty(int(n.value))
    call(t, b, int(n.value))
    return t, b, int(n.value)
