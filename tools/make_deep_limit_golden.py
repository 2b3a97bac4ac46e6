"""Writes tests/golden/deep_limit_eri.npz: the oracle's dense (ab|cd) tensor of the 45-primitive limit basis of
tests/test_deep_contractions_cpu.py (limit_shells: a 45-primitive s and p on one centre, one primitive s and p on the other,
R = 2.0), with the tables it was computed from.  The (pp|pp) quartet of the deep centre alone is 4.1e6 primitive quartets and
takes the oracle ~8 s, too long for a test that runs with every suite; tests/test_gpu_deep_contractions.py reads the tensor from
here and recomputes the cheap quartets at test time.

    python tools/make_deep_limit_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle import basis as ob, natives as nat
    from tests.test_deep_contractions_cpu import ORIGIN, SKEW, limit_shells
    t = ob.make_tables(([5, 1], np.stack([ORIGIN, ORIGIN + 2.0 * SKEW])), limit_shells())
    eri = nat.int2e(t)
    out = os.path.join(ROOT, "tests", "golden", "deep_limit_eri.npz")
    np.savez_compressed(out, eri=eri, atm=t.atm, bas=t.bas, env=t.env)
    print("wrote %s: nao %d, max |(ab|cd)| %.6f, %d bytes" % (out, t.nao, np.abs(eri).max(), os.path.getsize(out)))


if __name__ == "__main__":
    main()
