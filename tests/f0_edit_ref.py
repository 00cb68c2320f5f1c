"""Float64 numpy restatement of the prosody-control kernels as include/hsp.h states them: the pitch edit of log-F0 rows
(hsp_f0_edit_rows_f32) and the scaled durations (hsp_duration_scaled_f32).  The references of
tests/test_prosody_controls_host.py (properties), tests/test_gpu_f0_edit.py and tests/test_gpu_duration_scaled.py."""
import numpy as np

LN2_12 = np.log(2.0) / 12.0
ULP_BELOW_8 = 4.8e-7       # one fp32 ulp of a value in [4, 8): 2^-21 = 4.77e-7 (f_max <= 2.9 kHz keeps log(f + 1) < 8)


def hz_to_l(hz):
    """The track's unit: log(f0 + 1); 0 Hz (unvoiced) -> 0."""
    return np.log1p(np.asarray(hz, dtype=np.float64))


def l_to_hz(l):
    return np.expm1(np.asarray(l, dtype=np.float64))


def edit_row(l, n_b=None, shift=0.0, range_=1.0, target_hz=None, offsets=None, f_min=55.0, f_max=1100.0):
    """One row: ``l`` [n] (fp32 values) -> (out float64 [n], mean_hz).  ``offsets`` None is the header's NULL;
    ``target_hz`` None or <= 0: no target.  The float operands are taken at their fp32 values, as the kernel reads them."""
    l = np.asarray(l, dtype=np.float32)
    n = l.shape[0]
    n_b = n if n_b is None else min(max(int(n_b), 0), n)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    shift, range_, f_min, f_max = f32(shift), f32(range_), f32(f_min), f32(f_max)
    target = 0.0 if target_hz is None else f32(target_hz)
    out = np.zeros(n, dtype=np.float64)
    voiced = np.zeros(n, dtype=bool)
    voiced[:n_b] = l[:n_b] > 0
    p = np.log(np.expm1(l[voiced].astype(np.float64)))
    m = float(p.mean()) if p.size else 0.0
    mean_hz = float(np.exp(m)) if p.size else 0.0
    if shift == 0.0 and range_ == 1.0 and not target > 0 and offsets is None:     # identity: copied, no clamp
        out[:n_b] = l[:n_b]
        return out, mean_hz
    c = np.log(target) if target > 0 else m
    steps = shift + (np.asarray(offsets, dtype=np.float32)[:n][voiced].astype(np.float64) if offsets is not None else 0.0)
    q = c + range_ * (p - m) + steps * LN2_12
    q = np.minimum(np.maximum(q, np.log(f_min)), np.log(f_max))
    out[voiced] = np.log1p(np.exp(q))
    return out, mean_hz


def edit_rows(l, lengths=None, shift=None, range_=None, target_hz=None, offsets=None, f_min=55.0, f_max=1100.0):
    """[B, n] -> (out float64 [B, n], mean_hz float64 [B]); the per-row operands [B] or None, ``offsets`` [B, n] or
    None.  Row by row: a row's result cannot depend on the other rows."""
    l = np.asarray(l, dtype=np.float32)
    B = l.shape[0]
    rows = [edit_row(l[b], None if lengths is None else lengths[b], 0.0 if shift is None else shift[b],
                     1.0 if range_ is None else range_[b], None if target_hz is None else target_hz[b],
                     None if offsets is None else offsets[b], f_min, f_max) for b in range(B)]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])


def scaled_durations(value, lengths, scale, length_scale=None):
    """hsp_duration_scaled_f32 with numpy's ceil on the fp32 products formed in the stated order.  ``value`` fp32 [B, N]:
    expf(logw) as the device formed it (``length_scale`` a float: predicted durations, (value * length_scale) * scale),
    or the caller's durations (``length_scale`` None: value * scale).  -> (dur fp32 [B, N], frames fp32 [B])."""
    v = np.asarray(value, dtype=np.float32)
    s = np.asarray(scale, dtype=np.float32)
    if length_scale is not None:
        v = (v * np.float32(length_scale)).astype(np.float32)
    d = np.ceil((v * s).astype(np.float32)).astype(np.float32)
    d[np.arange(v.shape[1])[None, :] >= np.asarray(lengths).reshape(-1, 1)] = 0.0
    return d, d.sum(axis=1, dtype=np.float64).astype(np.float32)


def track(n, seed, voiced=0.7, centre_hz=160.0, spread=0.25):
    """A synthetic fp32 track [n]: voiced stretches of a wandering contour around ``centre_hz`` (ln-Hz standard deviation
    ``spread``), zeros between them."""
    r = np.random.default_rng(seed)
    walk = np.cumsum(r.standard_normal(n)) * 0.02
    hz = centre_hz * np.exp(spread * np.sin(np.arange(n) / 17.0 + r.uniform(0, 6)) + walk - walk.mean() if n else walk)
    on = (np.sin(np.arange(n) / 9.0 + r.uniform(0, 6)) < 2.0 * voiced - 1.0) if n else np.zeros(0, bool)
    return np.where(on, hz_to_l(hz), 0.0).astype(np.float32)
