"""Generates tests/golden/conv_dispatch.json.gz, the routing trace tests/test_gpu_dispatch.py compares against.

Needs a GPU.  The trace pins behaviour, so it is recorded from a tree known to route correctly and only re-recorded
on purpose (a deliberate routing change):
    python tests/golden/make_dispatch_golden.py
"""
import gzip
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_gpu_dispatch as td  # noqa: E402


def main():
    out = {}
    for name in td.SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            out[name] = td.capture(name, mp)
        print(name, len(out[name]["calls"]), "calls,", sum(len(p) for p in out[name]["plans"]), "planned launches",
              flush=True)
    with gzip.GzipFile(td.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(td.FIXTURE, os.path.getsize(td.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
