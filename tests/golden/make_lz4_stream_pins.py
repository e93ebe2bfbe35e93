#!/usr/bin/env python3
"""Records tests/golden/lz4_bytewise_streams.json: per case of tests/test_gpu_lz4_stream_pins.py and clevel, every stream's size
and SHA-256 as the byte-wise LZ4 coder (csrc/lz4.hip) writes them on the device.  Run it on the commit whose streams are to be
held, in two separate processes:

  python tests/golden/make_lz4_stream_pins.py --out first.json
  python tests/golden/make_lz4_stream_pins.py --against first.json

The second writes the fixture: a stream on which the two processes disagree is written as null and printed — the coder is
not deterministic there, which is a finding for the test module's docstring, not something to record."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from haplohyped_varawareml_amd.device import Context                      # noqa: E402
from tests.test_gpu_lz4_stream_pins import CASES, CLEVELS, FIXTURE, case_pins  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--against", help="an earlier recording: streams that differ from it are written as null")
    a = ap.parse_args()
    ctx = Context(0)
    rec = {f"{name}@{c}": case_pins(ctx, name, c) for name in sorted(CASES) for c in CLEVELS}
    ctx.close()
    n = sum(len(v) for v in rec.values())
    if a.against:
        first = json.load(open(a.against))
        assert sorted(first) == sorted(rec)
        bad = 0
        for key, pins in rec.items():
            assert len(pins) == len(first[key]), key
            for k, (p, q) in enumerate(zip(pins, first[key])):
                if p != q:
                    print(f"NOT DETERMINISTIC: {key} stream {k}: {q} then {p}")
                    pins[k] = None
                    bad += 1
        print(f"{bad} of {n} streams differ between the two recordings")
    with open(a.out, "w") as f:
        cases = [f'"{k}":[\n' + ",\n".join(json.dumps(p, separators=(",", ":")) for p in v) + "\n]" for k, v in sorted(rec.items())]
        f.write("{\n" + ",\n".join(cases) + "\n}\n")       # one stream per line
    print(f"wrote {a.out}: {len(rec)} cases, {n} streams")


if __name__ == "__main__":
    main()
