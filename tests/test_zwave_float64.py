"""Z-Wave R2 without a GPU: a second, independent statement of the front end z1-z4 (tests/zwave_ref.py restates the
kernels' own f32 arithmetic order, so an error both share -- mixing direction, discriminator gain, tap table, squelch
quantity -- would pass every bit-exact test).

Here the tap tables are checked as data against what firdes::low_pass(..., WIN_HAMMING) with the parameters of
ZWave_rx/top_block.py:42,66 implies, and the front end is written in float64 in GNU Radio 3.7's own form:
  freq_xlating_fir_filter_ccc  complex taps h1[k] exp(j theta k), theta = 2 pi (-200e3) / 800e3, output rotator
                               exp(-j theta n) (the rotator starts at phase 1 on the first output)
  simple_squelch_cc(-40, 1)    |y|^2 >= 10^(-40/10), alpha 1: the IIR average is the power itself
  quadrature_demod_cf          gain angle(y[n] conj y[n-1]), gain = 2 fs / (2 pi 20e3 / 8), y[-1] = 0 (zero history)
  fir_filter_fff               np.convolve with h2
and compared with the checker on clean captures and with known answers (tones) that hold for all three statements.
"""
import math
import os
import re

import numpy as np
import pytest

from snout_amd import zwave
import zwave_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 800e3
THETA = 2 * math.pi * (-200e3) / FS
GAIN = 2 * FS / (2 * math.pi * 20e3 / 8.0)
HALO = 39 + 193             # input samples that reach one f sample: x[n - 231 .. n]

# |f32 checker - float64| inside a frame (|y| ~ 1) or in silence (everything 0):
#  * the table-driven fast_atan2f interpolates atan linearly on steps of 1/255: error <= (1/255)^2 / 8 * max|atan''|
#    (0.65) = 1.3e-6 rad, times the gain (101.9) = 1.3e-4 in d, times sum |h2| (1.15) = 1.5e-4 in f;
#  * f32 rounding of y (39 products and sums at |y| ~ 1: <= 40 * 6e-8 relative) moves the angle by ~5e-6 rad: 5e-4 in d,
#    6e-4 in f at the worst, with all errors of one sign;
#  * the 193-tap f32 sum at |d| <= 24: <= 193 roundings of 24 * 6e-8 = 2.8e-4.
# Worst case about 1.1e-3; the bound is 2e-3.  (Measured on the captures below: 8.3e-5.)
TOL = 2e-3


def _inc_tables():
    """The committed tables, parsed as numbers (float64)."""
    text = open(os.path.join(ROOT, "snout_amd", "csrc", "zwave_taps.inc")).read()
    out = []
    for name in ("ZW_TAPS_XLATE", "ZW_TAPS_LP"):
        n = int(re.search(rf"#define {name}_N (\d+)", text).group(1))
        body = text.split(f"#define {name} \\")[1].split("\n\n")[0]
        vals = np.array([float(v) for v in re.findall(r"[-+]?\d\.\d+e[-+]\d+", body)], dtype=np.float64)
        assert vals.size == n
        out.append(vals)
    return out


def _response_db(h, nfft=1 << 16):
    H = np.abs(np.fft.rfft(h, nfft))
    return np.fft.rfftfreq(nfft, 1 / FS), 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("which, cutoff, tw, flat_to, stop_from, stop_db", [
    (0, 150e3, 50e3, 100e3, 200e3, -55.0),      # top_block.py:42  firdes.low_pass(1, fs, 150e3, 50e3, WIN_HAMMING)
    (1, 40e3, 10e3, 30e3, 50e3, -56.0),         # top_block.py:66  firdes.low_pass(1, fs, 40e3, 10e3, WIN_HAMMING, 6.76)
])
def test_tap_tables_meet_the_firdes_design(which, cutoff, tw, flat_to, stop_from, stop_db):
    h = _inc_tables()[which]
    assert h.size == int(53 * FS / (22 * tw)) | 1 == (39, 193)[which]
    f, db = _response_db(h)
    at = lambda hz: float(np.interp(hz, f, db))
    assert abs(at(cutoff) - (-6.0)) <= 0.1, at(cutoff)                  # a Hamming windowed sinc: half amplitude
    assert np.max(np.abs(db[f <= flat_to])) <= 0.05
    assert np.max(db[f >= stop_from]) <= stop_db
    assert abs(h.sum() - 1) < 1e-6                                      # gain 1 at DC


def front64(x):
    """z1-z4 in float64, GNU Radio's form -> (f, y after the squelch)."""
    h1, h2 = (h.astype(np.float64) for h in ref.taps())
    x = np.asarray(x).astype(np.complex128)
    n = x.size
    ctaps = h1 * np.exp(1j * THETA * np.arange(h1.size))
    y = np.convolve(x, ctaps)[:n] * np.exp(-1j * THETA * np.arange(n))
    y = np.where(np.abs(y) ** 2 >= 10 ** (-40 / 10), y, 0)
    prev = np.concatenate([[0], y[:-1]])
    d = GAIN * np.angle(y * np.conj(prev))
    return np.convolve(d, h2)[:n], y


def _steady(active):
    """Samples whose whole HALO-sample input window is all active or all inactive (x[< 0] counts as inactive)."""
    a = np.concatenate([np.zeros(HALO, np.int64), active.astype(np.int64)])
    c = np.concatenate([[0], np.cumsum(a)])
    s = c[HALO + 1:] - c[1:-HALO]             # active samples in x[n - 231 .. n]
    return (s == 0) | (s == HALO)


def tone(n, hz, amp=1.0, phase=0.3):
    return (amp * np.exp(1j * (phase + 2 * math.pi * hz / FS * np.arange(n)))).astype(np.complex64)


@pytest.mark.parametrize("seed", [3, 4])
def test_float64_front_end_against_the_checker_on_clean_captures(seed):
    x, truth = zwave.capture(1 << 16, seed=seed, sigma=0, mean_gap=3000.0)
    assert len(truth) >= 3
    f32, _, _ = ref.front(x)
    f64, _ = front64(x)
    ok = _steady(np.abs(x) > 0)
    inside = ok & (np.abs(x) > 0)
    assert inside.sum() > 20000 and (ok & (x == 0)).sum() > 5000
    err = np.abs(f32.astype(np.float64) - f64)
    assert np.max(err[ok]) <= TOL, float(np.max(err[ok]))
    assert np.all(f32[ok & (x == 0)] == 0) and np.all(np.abs(f64[ok & (x == 0)]) == 0)
    # the decisions the loop sees: FSK at +-20 kHz is f = +-16 in the middle of a run of equal bits
    assert np.max(np.abs(f32[inside])) > 15.0


@pytest.mark.parametrize("dk", [-30, -20, -5, 0, 5, 20, 30])
def test_tones_inside_the_channel_give_their_offset(dk):
    n = 4096
    x = tone(n, -200e3 + dk * 1e3)
    f32, _, _ = ref.front(x)
    f64, _ = front64(x)
    want = dk * 1e3 / 1250.0
    assert np.max(np.abs(f64[HALO:] - want)) <= TOL
    assert np.max(np.abs(f32[HALO:].astype(np.float64) - want)) <= TOL


@pytest.mark.parametrize("amp", [1.0, 5.0])
@pytest.mark.parametrize("off_khz", [-350, -300, -250, -200, 200, 250, 300, 350])
def test_tones_outside_the_channel_keep_the_squelch_closed(amp, off_khz):
    n = 4096
    x = tone(n, -200e3 + off_khz * 1e3, amp)
    f32, y32, _ = ref.front(x)
    f64, y64 = front64(x)
    # >= 55 dB down: amplitude 5 leaves |y|^2 <= 25 * 10^-5.5 = 7.9e-5, below the 1e-4 threshold
    assert np.all(y32[39:] == 0) and np.all(y64[39:] == 0)
    assert np.all(f32[HALO:] == 0.0) and np.all(f64[HALO:] == 0.0)


@pytest.mark.parametrize("dk", [-20, 5])
def test_weak_tones_inside_the_channel_close_and_open_the_squelch(dk):
    n = 4096
    weak = tone(n, -200e3 + dk * 1e3, 0.005)          # |y|^2 = 2.5e-5 < 1e-4
    f32, y32, _ = ref.front(weak)
    f64, y64 = front64(weak)
    assert np.all(y32 == 0) and np.all(y64 == 0) and np.all(f32 == 0.0) and np.all(f64 == 0.0)
    audible = tone(n, -200e3 + dk * 1e3, 0.02)        # |y|^2 = 4e-4
    f32, y32, _ = ref.front(audible)
    f64, y64 = front64(audible)
    assert np.all(y32[39:] != 0) and np.all(y64[39:] != 0)
    want = dk * 1e3 / 1250.0
    assert np.max(np.abs(f64[HALO:] - want)) <= TOL
    assert np.max(np.abs(f32[HALO:].astype(np.float64) - want)) <= TOL
