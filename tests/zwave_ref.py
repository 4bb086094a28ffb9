"""An independently written statement of the Z-Wave R2 receive chain z1-z7 (TEST INFRASTRUCTURE: the checker of
libsnout_rx.so's SNOUT_PROTO_ZWAVE path, bit for bit).

Written in numpy / plain Python from the reference flowgraph (snout/modulations/ZWave/hackrf/ZWave_rx/top_block.py:41-90)
and the arithmetic order DESIGN.md section 9 states:

  z1  u[m] = j^m x[m];  y[n] = sum_k h1[k] u[n-k], real and imaginary part apart, tap order k = 0..38, every product
      and every sum rounded to f32 (acc = 0; acc = acc + h1[k] v);  x[m < 0] = 0
  z2  p = re re + im im (f32); y[n] kept if float64(p) >= 1e-4, else 0
  z3  d[n] = f32(g) * quad_demod(y)[n]  (quad_demod: tests/zb_sequential_ref.py, the table-driven fast_atan2f)
  z4  f[n] = sum_k h2[k] d[n-k], tap order k = 0..192, rounded as z1
  z5  clock_recovery_mm_ff(20, 0.25 0.175^2, 0.5, 0.175, 0.005) as GNU Radio 3.7 steps it, the 802.15.4 path's MMSE
      bank (mmse_taps.inc), the 8-tap interpolation as an fma chain (each fma rounded once: exact product and sum in
      double, rounded to odd, then to f32)
  z6  bit = 0 if v < 0 else 1
  z7  the packet sink restated from G.9959 (24-bit register == 0x5555F0 starts a frame; byte 7 = L, 10..64; XOR checksum)

Two modes: sequential (one loop over the whole capture: the reference's receiver) and lanes (the shape the library runs:
lane k owns sample_index in [k C, (k + 1) C), starts max(0, k C - W) with a fresh loop and sink, goes past its core end
only to finish a frame it owns).  Taps come from snout_amd/csrc/zwave_taps.inc, the lane defaults from
include/snout_rx.h; the MMSE bank is passed in (the oracle fixture's copy, as tests/test_zigbee_sequential.py does).
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from zb_sequential_ref import quad_demod

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN = F(2 * 800000.0 / (2 * math.pi * 20e3 / 8.0))        # quadrature_demod_cf gain, top_block.py:74
OMEGA, GAIN_OMEGA, MU0, GAIN_MU, OMEGA_REL = 20.0, 0.25 * 0.175 * 0.175, 0.5, 0.175, 0.005    # top_block.py:69
SQUELCH = 10.0 ** (-40 / 10.0)                              # simple_squelch_cc(-40, 1): threshold in power
SYNC = 0x5555F0


def taps():
    """(h1, h2) as float32 arrays, parsed from the kernels' table."""
    text = open(os.path.join(ROOT, "snout_amd", "csrc", "zwave_taps.inc")).read()
    out = []
    for name in ("ZW_TAPS_XLATE", "ZW_TAPS_LP"):
        n = int(re.search(rf"#define {name}_N (\d+)", text).group(1))
        body = re.search(rf"#define {name} \\\n(.*?)\n\n", text, re.S).group(1)
        vals = [float(v) for v in re.findall(r"([-+0-9.eE]+)f,", body)]
        assert len(vals) == n
        out.append(np.array(vals, dtype=F))
    return tuple(out)


def lane_defaults():
    text = open(os.path.join(ROOT, "include", "snout_rx.h")).read()
    core = int(re.search(r"#define SNOUT_ZWAVE_LANE_CORE\s+(\d+)u", text).group(1))
    warm = int(re.search(r"#define SNOUT_ZWAVE_LANE_WARMUP\s+(\d+)u", text).group(1))
    return core, warm


def _fir(v: np.ndarray, h: np.ndarray) -> np.ndarray:
    """sum_k h[k] v[n-k], v[n < 0] = 0, in tap order, every product and sum rounded to f32."""
    acc = np.zeros(v.size, dtype=F)
    for k, hk in enumerate(h):
        sh = np.zeros(v.size, dtype=F)
        if k < v.size:
            sh[k:] = v[:v.size - k]
        acc = (acc + (F(hk) * sh).astype(F)).astype(F)
    return acc


def front(iq: np.ndarray):
    """z1-z4 -> (f, y after the squelch, d)."""
    h1, h2 = taps()
    x = np.ascontiguousarray(iq, dtype=np.complex64)
    re_, im_ = x.real.astype(F), x.imag.astype(F)
    r = np.arange(x.size) & 3                               # u = j^m x: exact sign flips and swaps
    ur = np.select([r == 0, r == 1, r == 2, r == 3], [re_, -im_, -re_, im_]).astype(F)
    ui = np.select([r == 0, r == 1, r == 2, r == 3], [im_, re_, -im_, -re_]).astype(F)
    yr, yi = _fir(ur, h1), _fir(ui, h1)
    pw = ((yr * yr).astype(F) + (yi * yi).astype(F)).astype(F)
    open_ = pw.astype(np.float64) >= SQUELCH
    y = np.where(open_, yr, F(0)).astype(F) + 1j * np.where(open_, yi, F(0)).astype(F)
    y = y.astype(np.complex64)
    d = (GAIN * quad_demod(y)).astype(F)
    f = _fir(d, h2)
    return f, y, d


def _fma(a, b, c):
    """f32 fma, one rounding: the exact product in double, the sum rounded to odd in double, then to f32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    cc = c.astype(np.float64)
    s = p + cc
    bp = s - p
    e = (p - (s - bp)) + (cc - bp)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0)
    up = (e > 0) == (s > 0)
    bits[fix] += np.where(up[fix], 1, -1)
    return bits.view(np.float64).astype(F)


def _mm(f: np.ndarray, starts: np.ndarray, limits: np.ndarray, mmse: np.ndarray):
    """z5 for every lane at once: lane i runs from starts[i] while its window fits the input and starts below limits[i].
    Returns per lane (symbol values f32, window start of every symbol)."""
    n = f.size
    L = starts.size
    ii = starts.astype(np.int64).copy()
    mu = np.full(L, F(MU0), dtype=F)
    omega = np.full(L, F(OMEGA), dtype=F)
    last = np.zeros(L, dtype=F)
    mid, lim = F(OMEGA), F(F(OMEGA) * F(OMEGA_REL))
    g_om, g_mu = F(GAIN_OMEGA), F(GAIN_MU)
    fpad = np.concatenate([f, np.zeros(8, dtype=F)])
    parts = []                                              # (lanes, symbols, window starts) of every step
    act = np.nonzero((ii + 8 <= n) & (ii < limits))[0]
    while act.size:
        a_ii, a_mu = ii[act], mu[act]
        imu = np.rint((a_mu * F(128.0)).astype(F)).astype(np.int64)
        rows = mmse[imu]
        acc = np.zeros(act.size, dtype=F)
        for k in range(8):                                  # acc = fma(taps[imu][k], f[ii + 7 - k], acc)
            acc = _fma(rows[:, k], fpad[a_ii + 7 - k], acc)
        o = acc
        parts.append((act, o, a_ii))
        la = last[act]
        s_last = np.where(la < 0, F(-1.0), F(1.0)).astype(F)
        s_o = np.where(o < 0, F(-1.0), F(1.0)).astype(F)
        mm = ((s_last * o).astype(F) - (s_o * la).astype(F)).astype(F)
        last[act] = o
        om = (omega[act] + (g_om * mm).astype(F)).astype(F)
        xo = (om - mid).astype(F)
        c = (F(0.5) * (np.abs((xo + lim).astype(F)) - np.abs((xo - lim).astype(F))).astype(F)).astype(F)
        om = (mid + c).astype(F)
        omega[act] = om
        m2 = ((a_mu + om).astype(F) + (g_mu * mm).astype(F)).astype(F)
        fl = np.floor(m2).astype(F)
        step = np.where(fl >= 1, fl.astype(np.int64), 1)
        ii[act] = a_ii + step
        mu[act] = (m2 - fl).astype(F)
        act = act[(ii[act] + 8 <= n) & (ii[act] < limits[act])]
    if not parts:
        return [np.zeros(0, F)] * L, [np.zeros(0, np.int64)] * L
    lane = np.concatenate([p[0] for p in parts])
    order = np.argsort(lane, kind="stable")               # per lane, in step order
    vals = np.concatenate([p[1] for p in parts])[order]
    where = np.concatenate([p[2] for p in parts])[order]
    cut = np.cumsum(np.bincount(lane, minlength=L))[:-1]
    return np.split(vals, cut), np.split(where, cut)


def _sink(vals, where, cs: int, ce: int, lane: int, first: int, channel: int):
    """z6 + z7 of one lane.  Returns (records, symbols the lane's loop computed before it stopped, stopped by the rule)."""
    reg, reading, owned = 0, False, False
    start = nb = nbits = cur = L = ptype = 0
    x = 0xFF
    buf = bytearray()
    recs = []
    for idx in range(vals.size):
        pos = int(where[idx])
        if pos >= ce and not (reading and owned):
            return recs, idx, True
        bit = 0 if vals[idx] < 0 else 1
        if not reading:
            reg = ((reg << 1) | bit) & 0xFFFFFF
            if reg == SYNC:
                reading, start, owned = True, pos, pos >= cs
                nb = nbits = cur = L = ptype = 0
                x = 0xFF
                buf = bytearray()
            continue
        cur = (cur << 1) | bit
        nbits += 1
        if nbits < 8:
            continue
        byte, cur, nbits = cur, 0, 0
        buf.append(byte)
        if nb == 5:
            ptype = byte & 0x0F
        if nb == 7:
            L = byte
        nb += 1
        if nb == 8 and (L < 10 or L > 64):
            reading, reg = False, 0
        elif nb >= 8 and nb == L:
            if owned:
                recs.append({"sample_index": first + start, "proto": 2, "channel": channel, "len": L,
                             "crc_ok": int(x == byte), "lqi": 0, "pdu_type": ptype, "flags": 0, "aux": lane,
                             "bytes": bytes(buf)})
            reading, reg = False, 0
        else:
            x ^= byte
    return recs, vals.size, False


def lanes(f: np.ndarray, mmse: np.ndarray, core: int, warmup: int, first: int = 0, channel: int = 0):
    """z5-z7 in lanes of `core` samples with `warmup` (core >= f.size: the sequential receiver).
    Returns (records in sample_index order, per lane its symbols up to where its loop stopped)."""
    n = f.size
    n_lanes = max(1, -(-n // core))
    cs = np.arange(n_lanes, dtype=np.int64) * core
    ce = np.minimum(cs + core, n)
    starts = np.maximum(cs - warmup, 0)
    limits = ce + 600 * 32                  # past the core end: at most one owned frame (64 bytes) to finish
    vals, where = _mm(f, starts, limits, mmse)
    recs, syms = [], []
    for k in range(n_lanes):
        r, used, stopped = _sink(vals[k], where[k], int(cs[k]), int(ce[k]), k, first, channel)
        assert stopped or where[k].size == 0 or where[k][-1] + 8 + 32 > n, "lane limit too short"
        recs += r
        syms.append(vals[k][:used])
    return recs, syms


def receive(iq: np.ndarray, mmse: np.ndarray, core: int = 0, warmup: int = 0, first: int = 0, channel: int = 0,
            sequential: bool = False):
    """The whole chain -> (records as dicts with the snout_pkt fields, f, per-lane symbols).  sequential=True: one loop
    over the capture; otherwise the lane shape (0: the library's defaults)."""
    f, _, _ = front(iq)
    if sequential:
        core, warmup = max(f.size, 1), 0
    else:
        dc, dw = lane_defaults()
        core, warmup = core or dc, warmup or dw
    recs, syms = lanes(f, mmse, core, warmup, first, channel)
    return recs, f, syms
