"""Whole-output float64 checker: every output sample of a many-source render, against the oracle's definition.

TEST INFRASTRUCTURE ONLY (as bas_oracle.py).  The FIR of each source is oracle/bas_oracle_fir.c
(libbas_oracle_fir.so, built by build()), driven over sources from a few threads through ctypes, which releases the
GIL; the chunk IRs come from bas_oracle.interp2d_many (bit-identical to interp2d) one source at a time, so that the
IRs of a whole scene are never resident at once.

Determinism: sources are taken in fixed groups of GROUP, each group accumulated in source order into a buffer of its
own, and the group sums added in group order - the result does not depend on the number of threads, bit for bit.
"""
import ctypes
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import bas_oracle as orc

GROUP = 8                  # sources per partial sum (fixed: the result must not depend on the thread count)
MAX_THREADS = 16
TILE = 8192                # output samples per tile of the FIR kernels

_lib = None
_lib_lock = threading.Lock()


def _fir():
    global _lib
    with _lib_lock:
        if _lib is None:
            lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbas_oracle_fir.so"))
            vp = ctypes.c_void_p
            lib.bas_oracle_render_accumulate.argtypes = [vp, ctypes.c_long, ctypes.c_int, ctypes.c_int, vp,
                                                         ctypes.c_int, vp]
            lib.bas_oracle_render_accumulate.restype = None
            _lib = lib
    return _lib


def default_threads():
    """At most 16, and at most OMP_NUM_THREADS where that is set."""
    n = MAX_THREADS
    env = os.environ.get("OMP_NUM_THREADS", "").strip()
    if env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return n


def irs_from_angles(tbl, elev, azim):
    """irs_of_source for per-source float64 angle rows (elev/azim [n_src, n_chunks + 1]): the source's chunk IRs."""
    def irs_of(i):
        return orc.interp2d_many(tbl, np.asarray(elev[i], dtype=np.float64), np.asarray(azim[i], dtype=np.float64))
    return irs_of


def render_mix_whole(signals, K, S, irs_of_source, threads=None):
    """float64 (2, T_out) un-normalised mix of every source's render (orc.render_mix's sum before the float32 cast).

    signals: a sequence (len() and [i]) of 1-D sources, all with the same padded length in_length = ceil(n / K) K
    (numpy rows, or a lazy object that makes source i on demand); irs_of_source(i) -> (in_length / K + 1, 2, L)
    float64 chunk IRs of source i.  threads: default_threads() when None, never more than 16."""
    assert K % S == 0
    n_src = len(signals)
    threads = default_threads() if threads is None else max(1, min(int(threads), MAX_THREADS))
    lib = _fir()
    first = np.asarray(signals[0])
    in_length = int(orc.render_lengths(first.size, K, 1)[0])
    L = int(np.asarray(irs_of_source(0)).shape[2])
    t_out = in_length + L - 1

    def group(g):
        acc = np.zeros((2, t_out))
        for i in range(g * GROUP, min((g + 1) * GROUP, n_src)):
            x = np.ascontiguousarray(signals[i], dtype=np.float64)
            assert x.ndim == 1 and orc.render_lengths(x.size, K, 1)[0] == in_length, "sources of different padded length"
            irs = np.ascontiguousarray(irs_of_source(i), dtype=np.float64)
            assert irs.shape == (in_length // K + 1, 2, L), irs.shape
            lib.bas_oracle_render_accumulate(x.ctypes.data, x.size, K, S, irs.ctypes.data, L, acc.ctypes.data)
        return acc

    n_groups = -(-n_src // GROUP)
    total = np.zeros((2, t_out))
    with ThreadPoolExecutor(threads) as ex:                 # at most 2 * threads partial sums pending at a time
        pending = []
        for g in range(n_groups):
            pending.append(ex.submit(group, g))
            if len(pending) >= 2 * threads:
                total += pending.pop(0).result()
        for f in pending:
            total += f.result()
    return total


def finish(acc, normalize):
    """What the product returns for the float64 mix `acc`: the float32 cast, then the peak rule when normalize
    (apply_hrtf.py:459-464, bas_oracle.render_mix).  Returned as float64 values of float32 numbers, (2, T_out)."""
    out = acc.astype(np.float32)
    if normalize:
        m = np.abs(out).max() if out.size else np.float32(0)
        if m > 1:
            out = out / m
    return out.astype(np.float64)


def compare(got, want, K, tile=TILE):
    """Norm-relative error over every sample of both ears (conftest.rel_err: max|got - want| / max|want|) and where
    the worst sample lies.  got / want: (2, T) arrays.  Returns a dict: rel, p9999 (the 99.99th percentile of
    |err| / max|want|), ear, n, n_mod_K, n_mod_tile, chunk, samples."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.ndim == 2 and got.shape[0] == 2, (got.shape, want.shape)
    err = np.abs(got - want)
    denom = float(np.abs(want).max()) if want.size else 0.0
    scale = denom if denom > 0 else 1.0
    flat = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    ear, n = divmod(flat, got.shape[1])
    worst = float(err.reshape(-1)[flat])
    return {"rel": worst / scale if not np.isnan(got).any() else float("nan"),
            "p9999": float(np.percentile(err, 99.99)) / scale,
            "ear": int(ear), "n": int(n), "n_mod_K": int(n % K), "n_mod_tile": int(n % tile), "chunk": int(n // K),
            "samples": int(got.size), "got": float(got[ear, n]), "want": float(want[ear, n]), "scale": denom}


def describe(res):
    """One line for a failure message: how far off and where."""
    return (f"rel err {res['rel']:.3e} (p99.99 {res['p9999']:.3e}) over {res['samples']} samples; worst at ear {res['ear']} "
            f"n={res['n']} (n mod K={res['n_mod_K']}, n mod tile={res['n_mod_tile']}, chunk {res['chunk']}): "
            f"got {res['got']:.9g}, want {res['want']:.9g}, scale {res['scale']:.6g}")


U32 = 2.0 ** -24            # the unit roundoff of float32
W_ROW = 32                  # one FIR row: the fast FIR forms x_e + x_o within a row


def widen_max(a, w):
    """max over |m - n| <= w of a[.., m], along the last axis (w = 0: a itself)."""
    a = np.asarray(a, dtype=np.float64)
    if w <= 0 or a.shape[-1] == 0:
        return a.copy()
    pad = [(0, 0)] * (a.ndim - 1) + [(w, w)]
    win = np.lib.stride_tricks.sliding_window_view(np.pad(a, pad), 2 * w + 1, axis=-1)
    return win.max(axis=-1)


def frame_max(a, Np, before=1, after=1):
    """The scale of a frame grid (the late tail): every sample of frame f = n // Np gets the maximum
    of a over the frames f - before .. f + after, along the last axis."""
    a = np.asarray(a, dtype=np.float64)
    T = a.shape[-1]
    nf = -(-T // Np)
    pad = [(0, 0)] * (a.ndim - 1) + [(0, nf * Np - T)]
    per = np.pad(a, pad).reshape(a.shape[:-1] + (nf, Np)).max(axis=-1)
    pad = [(0, 0)] * (a.ndim - 1) + [(before, after)]
    win = np.lib.stride_tricks.sliding_window_view(np.pad(per, pad), before + after + 1, axis=-1).max(axis=-1)
    return np.repeat(win, Np, axis=-1)[..., :T]


def local_scale(signals, K, S, irs_of_source, W=W_ROW, threads=None):
    """A_W, float64 (2, T_out): what float32 rounding of output sample n is measured against.
    A = render_mix_whole(|x|, K, S, |irs|) - the same C oracle fed absolute inputs and absolute chunk IRs; the crossfade
    weights are non-negative, so A[e, n] >= sum over sources and taps of |g[k]| |x[n - k]| - and
    A_W[e, n] = max over |m - n| <= W of A[e, m]."""
    class _Abs:
        def __len__(self):
            return len(signals)

        def __getitem__(self, i):
            return np.abs(np.asarray(signals[i], dtype=np.float64))

    A = render_mix_whole(_Abs(), K, S, lambda i: np.abs(np.asarray(irs_of_source(i), dtype=np.float64)), threads=threads)
    return widen_max(A, W)


def compare_local(got, want, scale, K=None, tile=TILE):
    """The worst ratio = |got - want| / (2^-24 scale) over the samples with scale > 0, and where it lies.  Half an ulp of
    float32(want) is taken off the error first: the output cast itself is not under test.  got / want / scale: arrays
    of one shape, the last axis time ((2, T) for a render, (T,) or (rows, T) for a row stage).  Returns a dict: ratio,
    zeros_ok (wherever scale == 0, got is exactly +-0), finite (no NaN or Inf in got), ear (the flat index of the
    leading axes), n, n_mod_K, n_mod_tile, chunk (None without K), got, want, scale (at the worst sample), samples,
    zeros (the samples with scale == 0)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    assert got.shape == want.shape == scale.shape and got.ndim >= 1, (got.shape, want.shape, scale.shape)
    T = got.shape[-1]
    got, want, scale = got.reshape(-1, T), want.reshape(-1, T), scale.reshape(-1, T)
    finite = bool(np.isfinite(got).all())
    half_ulp = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.maximum(np.abs(got - want) - half_ulp, 0.0)
    live = scale > 0
    ratio = np.zeros_like(err)
    np.divide(err, U32 * scale, out=ratio, where=live)
    ratio[live & ~np.isfinite(got)] = np.inf
    flat = int(np.argmax(ratio)) if ratio.size else 0
    ear, n = divmod(flat, T) if T else (0, 0)
    res = {"ratio": float(ratio.reshape(-1)[flat]) if ratio.size else 0.0,
           "zeros_ok": bool((got[~live] == 0).all()), "finite": finite,
           "ear": int(ear), "n": int(n), "n_mod_K": None if K is None else int(n % K), "n_mod_tile": int(n % tile),
           "chunk": None if K is None else int(n // K), "samples": int(got.size), "zeros": int((~live).sum())}
    if ratio.size:
        res.update(got=float(got[ear, n]), want=float(want[ear, n]), scale=float(scale[ear, n]))
    return res


def describe_local(res):
    """One line: how far off in units of 2^-24 of the local scale, and where."""
    return (f"ratio {res['ratio']:.3g} over {res['samples']} samples ({res['zeros']} of scale 0, zeros_ok {res['zeros_ok']}); "
            f"worst at row {res['ear']} n={res['n']} (n mod K={res['n_mod_K']}, n mod tile={res['n_mod_tile']}, chunk "
            f"{res['chunk']}): got {res.get('got', 0.0):.9g}, want {res.get('want', 0.0):.9g}, scale {res.get('scale', 0.0):.6g}")


def silent_support(signals, L, t_out=None):
    """Boolean mask of the output samples n whose whole input support [n - L + 1, n] is zero in every source (input
    samples past a source's end count as zero).  Length t_out, by default the longest source + L - 1."""
    n_max = max(np.asarray(signals[i]).size for i in range(len(signals)))
    t_out = n_max + L - 1 if t_out is None else int(t_out)
    nz = np.zeros(max(n_max, t_out), dtype=bool)
    for i in range(len(signals)):
        x = np.asarray(signals[i])
        nz[:x.size] |= x != 0
    c = np.concatenate([[0], np.cumsum(nz, dtype=np.int64)])
    n = np.arange(t_out)
    return (c[n + 1] - c[np.maximum(n - L + 1, 0)]) == 0
