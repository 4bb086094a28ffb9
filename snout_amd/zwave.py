"""Z-Wave R2 (ITU-T G.9959, 40 kbit/s NRZ 2-FSK): synthetic captures, the MPDU parse, and the scan handler that the
reference names but does not ship (snout/core/radio.py:50 and snout/cli.py:153-154 import ``snout.util.zwave``).

Captures are what the reference's flowgraph reads (snout/modulations/ZWave/hackrf/ZWave_rx/top_block.py): IQ at
800 ksps with the radio tuned to the channel + 200 kHz, so the signal sits at -200 kHz.  The receive chain itself is
libsnout_rx.so (proto SNOUT_PROTO_ZWAVE); tests/zwave_ref.py is its independent statement.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import _ffi
from .scan import _Events

FS = 800e3                    # top_block.py:41
OFFSET_HZ = -200e3            # the radio tunes to channel + 200 kHz (:55)
BAUD = 40e3                   # R2
DEVIATION_HZ = 20e3
SPS = int(FS / BAUD)          # 20 samples per bit
SOF = 0xF0
DEFAULT_MHZ = 908.4           # snout/util/__init__.py:16
MIN_LEN, MAX_LEN = 10, 64     # MPDU length byte: HomeID .. checksum
LINKTYPE_ZWAVE_R1_R2 = 261
# a scan cuts a capture into segments that overlap by the pre-roll (at least the lane warm-up, plus the FIR halos) and
# the longest frame on air; a segment leaves what it finds in its pre-roll to the segment before it
PREROLL = 16384 + 2048
LONGEST_FRAME = (20 + 1 + MAX_LEN) * 8 * SPS
OVERLAP = PREROLL + LONGEST_FRAME + 2048
SEGMENT = 1 << 22
DEDUP_TOL = 2 * SPS           # two runs of the timing loop over the same frame lock within a fraction of a symbol


def checksum(body: bytes) -> int:
    """G.9959 R1/R2 frame check: 0xFF XOR every byte from HomeID up to the checksum."""
    c = 0xFF
    for b in body:
        c ^= b
    return c


def make_mpdu(home_id: int, src: int, dst: int, payload: bytes, header_type: int = 1, seq: int = 0,
              routed: bool = False, ack: bool = False, low_power: bool = False) -> bytes:
    L = 10 + len(payload)
    if not MIN_LEN <= L <= MAX_LEN:
        raise ValueError(f"MPDU length {L} outside {MIN_LEN}..{MAX_LEN}")
    fc0 = (0x80 if routed else 0) | (0x40 if ack else 0) | (0x20 if low_power else 0) | (header_type & 0x0F)
    body = home_id.to_bytes(4, "big") + bytes([src & 0xFF, fc0, seq & 0x0F, L, dst & 0xFF]) + bytes(payload)
    return body + bytes([checksum(body)])


def parse_mpdu(mpdu: bytes) -> dict:
    """HomeID, source, destination, header type, routed / ack / low-power bits, sequence number, payload, checksum."""
    if len(mpdu) < MIN_LEN:
        raise ValueError("Z-Wave MPDU shorter than 10 bytes")
    L = mpdu[7]
    if L != len(mpdu):
        raise ValueError(f"length byte {L} != {len(mpdu)} bytes")
    fc0, fc1 = mpdu[5], mpdu[6]
    return {"home_id": int.from_bytes(mpdu[0:4], "big"), "src": mpdu[4], "dst": mpdu[8],
            "header_type": fc0 & 0x0F, "routed": bool(fc0 & 0x80), "ack": bool(fc0 & 0x40),
            "low_power": bool(fc0 & 0x20), "seq": fc1 & 0x0F, "length": L, "payload": bytes(mpdu[9:L - 1]),
            "checksum": mpdu[L - 1], "checksum_ok": checksum(mpdu[:L - 1]) == mpdu[L - 1]}


def frame_bits(mpdu: bytes, preamble: int = 10) -> np.ndarray:
    """Preamble (0x55 bytes), SOF 0xF0, MPDU: bits MSB first."""
    raw = bytes([0x55] * preamble + [SOF]) + bytes(mpdu)
    return np.unpackbits(np.frombuffer(raw, dtype=np.uint8))


def modulate(bits: np.ndarray, phase: float = 0.0, cfo_hz: float = 0.0) -> np.ndarray:
    """NRZ 2-FSK, +-20 kHz (bit 1 = positive deviation), 20 samples per bit, continuous phase, at -200 kHz + cfo."""
    f = np.repeat(np.where(np.asarray(bits) > 0, DEVIATION_HZ, -DEVIATION_HZ), SPS) + OFFSET_HZ + cfo_hz
    ph = phase + 2.0 * np.pi * np.cumsum(f) / FS
    return np.exp(1j * ph).astype(np.complex64)


@dataclass
class Truth:
    start: int          # first sample of the preamble
    sof_end: int        # last sample of the SOF's last bit
    mpdu: bytes


def random_mpdu(rng: np.random.Generator) -> bytes:
    L = int(rng.integers(MIN_LEN, MAX_LEN + 1))
    return make_mpdu(int(rng.integers(0, 1 << 32)), int(rng.integers(1, 233)), int(rng.integers(1, 256)),
                     rng.integers(0, 256, L - 10, dtype=np.uint8).tobytes(), header_type=int(rng.choice([1, 2, 3, 8])),
                     seq=int(rng.integers(0, 16)), routed=bool(rng.integers(0, 2)), ack=bool(rng.integers(0, 2)),
                     low_power=bool(rng.integers(0, 2)))


def capture(n: int, seed: int = 1, mean_gap: float = 6000.0, sigma: float = 0.05, cfo_hz: float = 500.0,
            max_frames: Optional[int] = None):
    """A seeded synthetic capture of n samples (complex64) with random valid frames (preambles of 10-20 bytes) at random
    gaps, each with its own random phase and a carrier offset in [-cfo_hz, cfo_hz]; AWGN of sigma per component."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.complex64)
    truth: List[Truth] = []
    pos = int(rng.integers(200, 2000))
    while max_frames is None or len(truth) < max_frames:
        mpdu = random_mpdu(rng)
        pre = int(rng.integers(10, 21))
        w = modulate(frame_bits(mpdu, pre), phase=float(rng.uniform(0, 2 * np.pi)),
                     cfo_hz=float(rng.uniform(-cfo_hz, cfo_hz)))
        if pos + w.size > n:
            break
        x[pos:pos + w.size] = w
        truth.append(Truth(pos, pos + (pre + 1) * 8 * SPS - 1, mpdu))
        pos += w.size + int(rng.exponential(mean_gap)) + 200
    if sigma:
        x += (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return x, truth


@dataclass
class ZWaveMessage:
    """One received Z-Wave frame (MPDU from HomeID through the checksum)."""
    mpdu: bytes
    timestamp: float
    mhz: float
    sample_index: int
    home_id: int
    src: int
    dst: int
    header_type: int
    seq: int
    routed: bool
    ack: bool
    low_power: bool
    payload: bytes
    protocol: str = "zwave"

    @classmethod
    def fromrecord(cls, p, t0: float, mhz: float) -> Optional["ZWaveMessage"]:
        """None unless the frame's checksum holds (as BtleMessage requires CRC0)."""
        if not int(p["crc_ok"]):
            return None
        mpdu = bytes(p["bytes"][:int(p["len"])])
        h = parse_mpdu(mpdu)
        si = int(p["sample_index"])
        return cls(mpdu=mpdu, timestamp=t0 + si / FS, mhz=mhz, sample_index=si, home_id=h["home_id"], src=h["src"],
                   dst=h["dst"], header_type=h["header_type"], seq=h["seq"], routed=h["routed"], ack=h["ack"],
                   low_power=h["low_power"], payload=h["payload"])

    def line(self) -> str:
        return (f"{self.timestamp:.6f} {self.mhz:.2f}MHz home={self.home_id:08x} src={self.src} dst={self.dst} "
                f"type={self.header_type} seq={self.seq} len={len(self.mpdu)} {self.mpdu.hex()}")


def fresh(rec, own_from: int, recent):
    """Indices of the records of a segment that are its own (sample_index >= own_from) and were not reported by the
    segment before (``recent``: its (sample_index, bytes)); returns them and this segment's (sample_index, bytes)."""
    keep, now = [], []
    for i, p in enumerate(rec):
        si, body = int(p["sample_index"]), bytes(p["bytes"][:p["len"]])
        if si < own_from or any(abs(si - s0) <= DEDUP_TOL and body == b0 for s0, b0 in recent):
            continue
        now.append((si, body))
        keep.append(i)
    return keep, now


def segments(x: np.ndarray, sample_format: int = 0, device: int = -1, **rx_kw):
    """A capture (complex64, or [n, 2] int8 / int16) through libsnout_rx.so in overlapping segments; yields the record
    array of every segment, in capture order, what a segment found in its pre-roll and what the segment before
    reported already (same bytes, sample_index within DEDUP_TOL) removed."""
    from .rx import SnoutRx
    n = len(x)
    recent = []
    with SnoutRx(proto=_ffi.PROTO_ZWAVE, channel=rx_kw.pop("channel", 0), device=device, sample_format=sample_format,
                 **rx_kw) as rx:
        a = 0
        while True:
            s = max(0, a - OVERLAP)
            b = min(n, a + SEGMENT)
            chunk = np.ascontiguousarray(x[s:b])
            if chunk.dtype != np.complex64:
                chunk = chunk.reshape(-1)
            rec = rx.process(chunk, first_sample_index=s) if b > s else np.zeros(0, dtype=_ffi.PKT_DTYPE)
            own = s + PREROLL if s else 0
            keep, recent = fresh(rec, own, recent)
            yield rec[keep]
            if b >= n:
                return
            a = b


class ZWaveScan:
    """Passive Z-Wave R2 scan, the ``snout.util.zwave.ZWaveScan`` that snout/core/radio.py:50 expects: every frame with a
    good checksum becomes a :class:`ZWaveMessage`, is appended to ``packets`` and emitted as ``zwave.packet-received``;
    the stop conditions are the other scans' (``packet_threshold`` frames, ``timeout`` seconds of capture time -- or of
    the wall clock for a live stream)."""

    def __init__(self, source=None, mhz: float = DEFAULT_MHZ, timeout: Optional[float] = 10.0,
                 packet_threshold: Optional[int] = None, t0_epoch: Optional[float] = None, device: int = -1,
                 rx_kw: Optional[Dict] = None):
        self.source = source
        self.mhz = mhz
        self.timeout = timeout
        self.packet_threshold = packet_threshold
        self.t0_epoch = time.time() if t0_epoch is None else t0_epoch
        self.device = device
        self.rx_kw = dict(rx_kw or {})
        self.packets: List[ZWaveMessage] = []
        self.events = _Events()
        self._elapsed = 0.0

    def frames(self):
        if hasattr(self.source, "segments"):         # a live stream: segments as they arrive, timeout by the wall clock
            t_start = time.time()
            for rec in self.source.segments(_ffi.PROTO_ZWAVE, 0, self.device, **self.rx_kw):
                for p in rec:
                    self._elapsed = time.time() - t_start
                    yield p
                self._elapsed = time.time() - t_start
                if self.timeout and self._elapsed >= self.timeout:
                    return
            return
        x = self.source.read(0)
        for rec in segments(x, getattr(self.source, "sample_format", 0), self.device, **self.rx_kw):
            for p in rec:
                self._elapsed = int(p["sample_index"]) / FS
                yield p

    def run(self) -> List[ZWaveMessage]:
        self._elapsed = 0.0
        for p in self.frames():
            self.handle_packet(p)
            if self.check_stop():
                break
        return self.packets

    def handle_packet(self, p) -> bool:
        m = ZWaveMessage.fromrecord(p, self.t0_epoch, self.mhz)
        if m is None:
            return False
        self.packets.append(m)
        self.events.emit("zwave.packet-received", message=m)
        return True

    def check_stop(self) -> bool:
        if self.packet_threshold and len(self.packets) >= self.packet_threshold:
            return True
        if self.timeout and self._elapsed >= self.timeout:
            return True
        return False

