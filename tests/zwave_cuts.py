"""The Z-Wave scans' segmentation restated for the tests (TEST INFRASTRUCTURE), and captures with frames placed at the
cuts.

A scan runs the receiver over overlapping chunks [s, b) of the capture, each with first_sample_index = s.  A chunk owns
the records with sample_index >= s + PREROLL (the first chunk: all of them); of those it drops a record whose bytes equal a
record the chunk before kept, within DEDUP_TOL samples.  The two scans differ only in where they cut:
  file   (zwave.segments):       cut a_0 = 0, s = max(0, a - OVERLAP), b = min(n, a + SEGMENT), next a = b, up to b = n
  stream (StreamSource, Z-Wave): s_0 = 0, b = min(n, s + seg), next s = b - OVERLAP, up to b = n;
                                  seg = max(segment, 4 OVERLAP)
"""
from __future__ import annotations

import numpy as np

from snout_amd import _ffi, zwave

SPS = 20                                     # samples per bit at 800 ksps, 40 kbit/s
PREROLL = 16384 + 2048                       # the default lane warm-up plus the FIR halos
LONGEST = (20 + 1 + 64) * 8 * SPS            # the longest frame on air: 20 preamble bytes, SOF, a 64-byte MPDU
OVERLAP = PREROLL + LONGEST + 2048
DEDUP_TOL = 2 * SPS


def file_cuts(n: int, segment: int):
    cuts, a = [], 0
    while True:
        s, b = max(0, a - OVERLAP), min(n, a + segment)
        cuts.append((s, b, s + PREROLL if s else 0))
        if b >= n:
            return cuts
        a = b


def stream_cuts(n: int, segment: int):
    seg = max(segment, 4 * OVERLAP)
    cuts, s = [], 0
    while True:
        b = min(n, s + seg)
        if b > s:
            cuts.append((s, b, s + PREROLL if s else 0))
        if b >= n:
            return cuts
        s = b - OVERLAP


def compose(x: np.ndarray, cuts, receive, stats=None):
    """receive(chunk, first) -> records of the chunk (dicts or a PKT_DTYPE array); returns the kept records per chunk.
    stats (a dict): counts the records dropped as "preroll" and as "duplicate"."""
    out, recent = [], []
    stats = {} if stats is None else stats
    stats.setdefault("preroll", 0)
    stats.setdefault("duplicate", 0)
    for s, b, own in cuts:
        rec = receive(x[s:b], s)
        keep, now = [], []
        for p in rec:
            si, body = int(p["sample_index"]), bytes(p["bytes"][:int(p["len"])])
            if si < own:
                stats["preroll"] += 1
                continue
            if any(abs(si - s0) <= DEDUP_TOL and body == b0 for s0, b0 in recent):
                stats["duplicate"] += 1
                continue
            now.append((si, body))
            keep.append(p)
        recent = now
        out.append(keep)
    return out


def as_pkts(recs) -> np.ndarray:
    """Checker records (dicts) -> a PKT_DTYPE array, as the library returns them."""
    a = np.zeros(len(recs), dtype=_ffi.PKT_DTYPE)
    for i, r in enumerate(recs):
        for k in ("sample_index", "proto", "channel", "len", "crc_ok", "lqi", "pdu_type", "flags", "aux"):
            a[i][k] = r[k]
        a[i]["bytes"][:len(r["bytes"])] = np.frombuffer(r["bytes"], dtype=np.uint8)
    return a


def _frame(rng, L: int, pre: int = 10):
    body = zwave.make_mpdu(int(rng.integers(0, 1 << 32)), int(rng.integers(1, 233)), int(rng.integers(1, 256)),
                           rng.integers(0, 256, L - 10, dtype=np.uint8).tobytes(), seq=int(rng.integers(0, 16)))
    w = zwave.modulate(zwave.frame_bits(body, pre), phase=float(rng.uniform(0, 2 * np.pi)))
    return body, w, (pre + 1) * 8 * SPS          # the SOF's last bit ends this many samples after the frame's start


def placed_capture(cuts, n: int, seed: int, sigma: float = 0.01, edge: bool = False):
    """A capture of n samples with, at every cut but the first (s, b, own) and the chunk before it ending at a = its
    end:  a frame starting inside the pre-roll [s, s + PREROLL);  a frame whose SOF ends 100 samples before own (so that
    the two chunks' loops put its sample_index within a symbol of own, on either side);  and either (edge=False) a frame
    straddling the end of the chunk before, or (edge=True) a frame ending on its last sample.  Plus a frame in the middle
    of every chunk.  Returns (x, [(start, end, mpdu)] in capture order)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.complex64)
    placed = []

    def put(start, L):
        body, w, _ = _frame(rng, L)
        assert 0 <= start and start + w.size <= n
        assert all(start >= e + 300 or start + w.size + 300 <= s0 for s0, e, _ in placed), "frames overlap"
        x[start:start + w.size] = w
        placed.append((start, start + w.size, body))

    ends = [b for _, b, _ in cuts]
    for k in range(1, len(cuts)):
        s, _, own = cuts[k]
        a = ends[k - 1]                                  # the last sample of chunk k - 1 is a - 1
        put(s + 1000, 64)                                # in the pre-roll: chunk k - 1 reports it
        near = own - 100 - 11 * 8 * SPS + 1              # SOF end at own - 100: sample_index (~100 later) within a symbol of own
        put(near, 10 if edge else 30)
        if edge:
            put(a - (11 + 40) * 8 * SPS, 40)             # ends on sample a - 1: only chunk k can finish it
        else:
            put(a - 3000, int(rng.integers(20, 65)))     # straddles the cut
    for s, b, _ in cuts:                                 # one frame well inside every chunk
        mid = (s + b) // 2
        if all(mid >= e + 300 or mid + LONGEST + 300 <= s0 for s0, e, _ in placed) and mid + LONGEST < n:
            put(mid, int(rng.integers(10, 65)))
    if sigma:
        x += (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    placed.sort(key=lambda t: t[0])
    return x, placed
