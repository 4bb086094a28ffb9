#!/usr/bin/env python3
"""Generate the Z-Wave golden fixture under tests/golden/:

zwave_r2_800k.cf32         131 072 cf32 samples at 800 ksps (1 MiB), seed 1: R2 frames (2-FSK +-20 kHz, 40 kbaud NRZ) at
                           -200 kHz as the reference's receiver is tuned, preambles of 10-20 bytes, random valid MPDUs of
                           10-64 bytes, a random phase per frame, AWGN; no carrier offset (the
                           clock recovery can lock to the bit transitions of a preamble seen with an offset).
zwave_r2_expected.json     the generator's truth: every frame's MPDU and the sample of its SOF's last bit.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from snout_amd import zwave
    x, truth = zwave.capture(1 << 17, seed=1, sigma=0.03, cfo_hz=0.0)
    assert len(truth) >= 6
    x.tofile(os.path.join(HERE, "zwave_r2_800k.cf32"))
    doc = {"fs": zwave.FS, "seed": 1, "n_samples": int(x.size),
           "frames": [{"sof_end": t.sof_end, "start": t.start, "mpdu": t.mpdu.hex()} for t in truth]}
    with open(os.path.join(HERE, "zwave_r2_expected.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(truth)} frames")


if __name__ == "__main__":
    main()
