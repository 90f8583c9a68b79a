"""Generates tests/golden/conv_fp32_bits.json.gz, the recording tests/test_gpu_conv_fp32_bits.py compares against.

Needs a GPU.  The recording pins the bits of the fp32-matrix-pipe convolutions and their weight packers, so it is made from a library known to
compute them correctly and only re-made on purpose (a deliberate change of their arithmetic):
    python tests/golden/make_conv_fp32_bits_golden.py
Every case is run twice; nothing is written unless the two runs agree in every bit.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_gpu_conv_fp32_bits as tb  # noqa: E402


def main():
    out = {}
    for name in tb.CASES:
        first, second = tb.record(name), tb.record(name)
        if first != second:
            sys.exit(f"{name}: two runs differ in {sorted(k for k in first if first[k] != second[k])}; nothing written")
        out[name] = first
        print(name, len(first), "records", flush=True)
    with gzip.GzipFile(tb.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
    print(tb.FIXTURE, os.path.getsize(tb.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
