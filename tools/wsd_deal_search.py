"""Offline search for the tile ownership of vxc_wsd_kernel (csrc/grid_vxc.hip: WSD_OWNER).

A block owns the upper triangle of the T x T output tiles (10 <= T <= 13) and deals it to 8 consumer waves.  A wave that owns
the tile set S reads, per k-group, the Phi and the Psi fragment of every tile index that occurs in S as a row or as a column:
2 |U(S)| ds_read_b64.  The search (simulated annealing over the owner of every tile) minimises sum_w |U_w| under

  * at most 12 tiles per wave (the accumulator registers),
  * |U_w| <= 7 (two fragment sets of 4 |U| registers beside 96 accumulator registers within 168 VGPRs),
  * MFMAs per k-group (2 per off-diagonal tile, 1 per diagonal tile) of the SIMDs {w, w + 4} differ by at most one,
  * the two waves of a SIMD differ by at most 2 MFMAs (a wave that runs alone issues at less than half the rate).

Prints the table as C++ rows (owner of every upper-triangle tile, row-major with the diagonal) and the figures the
static_asserts in grid_vxc.hip state.  Deterministic for a given --seed.

    python tools/wsd_deal_search.py [--seed 1] [--iters 300000]
"""
import argparse
import math
import random

NW = 8


def tiles_of(T):
    return [(i, j) for i in range(T) for j in range(i, T)]


def figures(T, own):
    tl = tiles_of(T)
    nt = [0] * NW
    mf = [0] * NW
    us = [set() for _ in range(NW)]
    for (i, j), w in zip(tl, own):
        nt[w] += 1
        mf[w] += 1 if i == j else 2
        us[w].add(i)
        us[w].add(j)
    return nt, mf, [len(u) for u in us]


def cost(T, own):
    nt, mf, nu = figures(T, own)
    simd = [mf[q] + mf[q + 4] for q in range(4)]
    c = float(sum(nu))
    c += 50.0 * sum(max(0, n - 12) for n in nt)
    c += 50.0 * sum(max(0, n - 7) for n in nu)
    c += 20.0 * max(0, max(simd) - min(simd) - 1)
    c += 20.0 * sum(max(0, abs(mf[q] - mf[q + 4]) - 2) for q in range(4))
    return c


def feasible(T, own):
    nt, mf, nu = figures(T, own)
    simd = [mf[q] + mf[q + 4] for q in range(4)]
    return (max(nt) <= 12 and max(nu) <= 7 and max(simd) - min(simd) <= 1
            and all(abs(mf[q] - mf[q + 4]) <= 2 for q in range(4)))


def search(T, seed, iters):
    rng = random.Random(seed * 100 + T)
    n = T * (T + 1) // 2
    own = [u * NW // n for u in range(n)]
    cur = cost(T, own)
    best, best_own = (cur, list(own)) if feasible(T, own) else (math.inf, None)
    for it in range(iters):
        temp = 2.0 * (1.0 - it / iters) + 0.05
        a = rng.randrange(n)
        if rng.random() < 0.5:
            b, old = None, own[a]
            own[a] = rng.randrange(NW)
        else:
            b = rng.randrange(n)
            own[a], own[b] = own[b], own[a]
        new = cost(T, own)
        if new <= cur or rng.random() < math.exp((cur - new) / temp):
            cur = new
            if cur < best and feasible(T, own):
                best, best_own = cur, list(own)
        elif b is None:
            own[a] = old
        else:
            own[a], own[b] = own[b], own[a]
    return best_own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--iters", type=int, default=300000)
    args = ap.parse_args()
    for T in range(10, 14):
        own = search(T, args.seed, args.iters)
        if own is None:
            raise SystemExit(f"T = {T}: no feasible deal found")
        nt, mf, nu = figures(T, own)
        print(f"    // T = {T}: tiles {nt}, MFMAs {mf}, SIMDs {[mf[q] + mf[q + 4] for q in range(4)]}, |U| {nu}, "
              f"sum |U| = {sum(nu)} (linear deal: {T * T} fragment pairs)")
        print("    {" + ", ".join(str(w) for w in own) + "},")
        tl = tiles_of(T)
        for i in range(T):
            print("    //   " + "  " * i + " ".join(str(own[tl.index((i, j))]) for j in range(i, T)))


if __name__ == "__main__":
    main()
