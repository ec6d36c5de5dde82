"""TEST INFRASTRUCTURE ONLY - finds the quads of the noise generator whose Philox output lies at an end of the uniform range, and writes
them to tests/golden/rng_edges.json (data only: keying tuples, the four counter words, the classes).  Each end has probability below
2^-24 per draw, so no statistical test ever reaches it; the tests evaluate the kernel AT these tuples instead.

    python -m oracle.find_rng_edges            (CPU, numpy; a few seconds per 10^7 quads)

Classes of a quad (c = its four Philox output words; c[0], c[2] feed the radii, c[1], c[3] the angles):
  a  a radius word below 2^10: the far tail, |z| up to sqrt(-2 ln 2^-33) = 6.764
  b  a radius word >= 2^32 - 128: float(c) rounds to 2^32 and only the clamp keeps u below 1 (ln u = 0 would give z = 0 exactly, u > 1 a NaN)
  c  an angle word >= 2^32 - 128: u = 1.0, the angle is the float32 2 pi itself
  d  a radius word in [2^23, 2^24): the `+ 0.5f` rounds (ulp 1)

The scan walks (seed, sample, step) in a fixed order with q < 2^18 each, and stops once every class has MIN_PER_CLASS tuples (classes b
and c have 2^-24 per quad: about 2 * 10^7 quads per hit).
"""
from __future__ import annotations

import itertools
import json
import os

import numpy as np

from . import rng_ref

NQ = 1 << 18
MIN_PER_CLASS, MAX_PER_CLASS = 2, 3
STEPS = (-1, 0, 1, 999)
SAMPLES = (0, 1, 5, (1 << 32) + 3)
TOP = (1 << 32) - 128


def classes_of(c):
    """The sorted class letters of one quad's counter words (ints)."""
    out = set()
    for r in (c[0], c[2]):
        if r < (1 << 10): out.add("a")
        if r >= TOP: out.add("b")
        if (1 << 23) <= r < (1 << 24): out.add("d")
    for a in (c[1], c[3]):
        if a >= TOP: out.add("c")
    return sorted(out)


def scan(max_quads=1 << 31):
    found = {k: [] for k in "abcd"}
    tuples, seen, done = [], set(), 0
    q = np.arange(NQ, dtype=np.uint64)
    for seed, sample, step in ((s, m, t) for s in itertools.count(0) for m in SAMPLES for t in STEPS):
        if all(len(v) >= MIN_PER_CLASS for v in found.values()) or done >= max_quads:
            break
        c = rng_ref.noise_counters(seed, sample, step, q)
        done += NQ
        rad = [c[0], c[2]]
        hit = np.zeros(NQ, bool)
        for r in rad:
            hit |= (r < np.uint64(1 << 10)) | (r >= np.uint64(TOP))
            if len(found["d"]) < MAX_PER_CLASS:
                hit |= (r >= np.uint64(1 << 23)) & (r < np.uint64(1 << 24))
        for a in (c[1], c[3]):
            hit |= a >= np.uint64(TOP)
        for i in np.nonzero(hit)[0]:
            words = [int(w[i]) for w in c]
            cls = classes_of(words)
            if not any(len(found[k]) < MAX_PER_CLASS for k in cls):
                continue
            key = (seed, sample, step, int(i))
            if key in seen:
                continue
            seen.add(key)
            for k in cls:
                found[k].append(key)
            tuples.append(dict(seed=seed, sample=sample, step=step, q=int(i), counters=words, classes=cls))
    return tuples, done


def main():
    tuples, done = scan()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "golden", "rng_edges.json")
    with open(path, "w") as f:
        json.dump({"quads_scanned": done, "quads_per_stream": NQ, "tuples": tuples}, f, indent=1)
        f.write("\n")
    per = {k: sum(k in t["classes"] for t in tuples) for k in "abcd"}
    print(f"{len(tuples)} tuples from {done} quads, per class {per} -> {path}")


if __name__ == "__main__":
    main()
