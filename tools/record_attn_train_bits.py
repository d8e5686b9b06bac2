#!/usr/bin/env python3
"""Record the fixture of tests/test_attn_train_bits_gpu.py: SHA-256 of the
attention train kernels' O, lse, dQ, dK and dV and of the seeded inputs.

Run on an MI355X with the kernel library built from the commit whose
outputs are the standard (the parent of the change under test):

    python tools/record_attn_train_bits.py [--out PATH]

The default PATH is tests/golden/attn_train_bits.json.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import test_attn_train_bits_gpu as bits

    p = argparse.ArgumentParser()
    p.add_argument("--out", default=bits.GOLDEN)
    args = p.parse_args()
    rec = bits.record()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases -> %s" % (len(rec), args.out))


if __name__ == "__main__":
    main()
