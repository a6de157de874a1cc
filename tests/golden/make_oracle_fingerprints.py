#!/usr/bin/env python3
"""Generates tests/golden/oracle_fingerprints.json: bit patterns of what the CPU oracle computes in a dozen configurations at
2..16 haplotypes (tests/oracle_fingerprints.py lists them and says what is kept).

    python tests/golden/make_oracle_fingerprints.py        (CPU only; a few seconds)

The committed file was written with the oracle as it stood BEFORE it was widened from 16 to 64 haplotypes, so that
tests/test_oracle_wide_cpu.py::test_oracle_at_16_or_fewer_is_unchanged shows that widening moved nothing.  Regenerate it only
when the oracle's results at n <= 16 are meant to change, and say so in that commit.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_fingerprints  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    out = {"generator": "tests/golden/make_oracle_fingerprints.py", "configurations": {}}
    for cfg in oracle_fingerprints.CONFIGS:
        fp = oracle_fingerprints.fingerprint(oracle_lib, cfg[0])
        out["configurations"][cfg[0]] = fp
        print(cfg[0], "rows", fp.get("rows"), "resamplings", fp.get("resamplings"), flush=True)
    with open(os.path.join(ROOT, "tests/golden/oracle_fingerprints.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
