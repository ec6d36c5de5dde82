"""The numpy restatements of the noise generator and of the dropout keep-mask (oracle/rng_ref.py), checked on the CPU against what is
known independently of this project: the published Philox4x32-10 known-answer vectors, the exact normal distribution, the binomial law.
tests/test_gpu_rng.py then holds the HIP kernels to the restatement value by value.  Every input is fixed: nothing here is flaky.

Statistical bounds: every statistic is divided by its own standard error under the null and bounded by 6 (two-sided normal tail 2e-9);
the Kolmogorov-Smirnov distance by D sqrt(n) < 3.27, i.e. 2 exp(-2 D^2 n) = 1e-9."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import find_rng_edges, rng_ref as R

SIGMAS = 6.0
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rng_edges.json")


def hexwords(s):
    return [int(w, 16) for w in s.split()]


# ------------------------------------------------------------------------------------------------ vectors and fixture
@pytest.mark.parametrize("counter,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answer_vectors(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = R.philox4x32_10(hexwords(counter), hexwords(key))
    assert [int(w) for w in got] == hexwords(want)
    many = R.philox4x32_10([np.full(5, w, np.uint64) for w in hexwords(counter)], hexwords(key))          # the vectorised form
    assert all((np.asarray(m) == w).all() for m, w in zip(many, hexwords(want)))


def load_edges():
    with open(EDGES) as f:
        return json.load(f)["tuples"]


def test_edge_fixture_holds_the_stated_counters_and_classes():
    tuples = load_edges()
    for cls in "abcd":
        assert sum(cls in t["classes"] for t in tuples) >= 2, cls
    for t in tuples:
        assert 0 <= t["q"] < (1 << 18)
        c = R.noise_counters(t["seed"], t["sample"], t["step"], np.array([t["q"]], np.uint64))
        words = [int(w[0]) for w in c]
        assert words == t["counters"], t
        assert find_rng_edges.classes_of(words) == t["classes"], t
        u0, a0, u2, a1 = R.uniforms(c)
        for cw, u in ((words[0], u0), (words[2], u2)):
            assert 0.0 < u[0] < 1.0
            if cw >= (1 << 32) - 128:
                assert u[0] == R.U_MAX                                # class b: float(c) + 0.5f is 2^32; the clamp alone keeps u < 1
        for cw, a in ((words[1], a0), (words[3], a1)):
            if cw >= (1 << 32) - 128:
                assert a[0] == R.TWO_PI_F32                           # class c: u = 1.0
        z32, z64 = R.box_muller(u0, a0, u2, a1)
        assert np.isfinite(z64).all() and np.isfinite(z32).all()
        assert np.abs(z64).max() <= 6.764                             # sqrt(-2 ln 2^-33) = 6.7638
        if "a" in t["classes"]:
            assert max(np.hypot(z64[0, 0], z64[0, 1]), np.hypot(z64[0, 2], z64[0, 3])) > 5.5          # radius of a word below 2^10


def test_float_stage_rounds_as_the_kernel_does():
    """u32 -> f32 to nearest even, + 0.5f, * 2^-32, the clamp: the float32 values at the words where each of them rounds."""
    words = np.array([0, 1, (1 << 23) + 1, (1 << 24) - 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 32) - 129, (1 << 32) - 128, (1 << 32) - 1], np.uint64)
    zero = np.zeros_like(words)
    u0, a0, _, _ = R.uniforms((words, words, zero, zero))
    want_u = [2.0 ** -33, 1.5 * 2.0 ** -32, (2 ** 23 + 2) * 2.0 ** -32,          # 2^23 + 1.5 ties to even: 2^23 + 2
              2.0 ** -8, 2.0 ** -8, (2 ** 24 + 4) * 2.0 ** -32,                  # 2^24 - 0.5 -> 2^24; 2^24 + 1 -> 2^24; 2^24 + 3 -> 2^24 + 4
              1 - 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24]                     # 2^32 - 129 -> 2^32 - 256 (+ 0.5f: no change); the last two clamp
    assert u0.dtype == np.float32 and [float(x) for x in u0] == want_u
    assert float(a0[-1]) == float(R.TWO_PI_F32) and float(a0[0]) == 0.0


# ------------------------------------------------------------------------------------------------ keying
def test_noise_keys_of_nearby_seeds_and_samples_are_distinct():
    seed = np.arange(1024, dtype=np.uint64)[:, None]
    sample = np.arange(8192, dtype=np.int64)[None, :]
    k0, _ = R.noise_key(seed, sample)
    assert k0.shape == (1024, 8192) and np.unique(k0).size == 1 << 23


def test_every_part_of_the_keying_reaches_the_stream():
    q = np.arange(256, dtype=np.uint64)
    base = np.stack(R.noise_counters(7, 0, 3, q))
    others = {"step + 1": (7, 0, 4), "step - 1": (7, 0, 2), "step = -1 (x_T)": (7, 0, -1), "step + 256": (7, 0, 259), "step + 65536": (7, 0, 65539),
              "seed + 1": (8, 0, 3), "high seed word": (7 + (1 << 32), 0, 3), "sample + 1": (7, 1, 3), "high sample word": (7, 1 << 32, 3),
              "negative sample": (7, -1, 3)}
    streams = {"base": base}
    for name, (seed, sample, step) in others.items():
        streams[name] = np.stack(R.noise_counters(seed, sample, step, q))
    names = list(streams)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            same = (streams[a] == streams[b]).mean()
            assert same < 0.01, (a, b, same)                          # 1024 words each: equal words are 2^-32 events
    # the high word of q is part of the counter as well
    hi = np.stack(R.noise_counters(7, 0, 3, q + np.uint64(1 << 32)))
    assert (hi == base).mean() < 0.01


def test_the_one_collision_of_the_keying_is_by_construction():
    """k0 = seed_lo ^ (uint32(sample) * 0x9E3779B1): the seed and the sample index share one 32-bit key word, so (seed ^ 0x9E3779B1,
    sample 0) and (seed, sample 1) are the same stream.  A property of the keying, recorded here so that nobody takes it for a fault of a
    kernel; seeds of one job differ in ways (small increments) for which test_noise_keys_of_nearby_seeds_and_samples_are_distinct holds."""
    q = np.arange(64, dtype=np.uint64)
    for seed in (0, 7, 0xDEADBEEF12345678):
        a = np.stack(R.noise_counters(seed ^ 0x9E3779B1, 0, 3, q))
        b = np.stack(R.noise_counters(seed, 1, 3, q))
        assert (a == b).all()


# ------------------------------------------------------------------------------------------------ distribution
def norm_cdf(x):
    return (0.5 * torch.special.erfc(-torch.from_numpy(np.asarray(x, np.float64)) / math.sqrt(2.0))).numpy()


def corr_z(a, b):
    """Sample correlation of a and b times sqrt(n): standard normal under independence."""
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / (a.std() * b.std()) * math.sqrt(a.size))


@pytest.fixture(scope="module")
def stream():
    _, z = R.normal_quads(7, 0, 3, np.arange(65536, dtype=np.uint64))
    z.setflags(write=False)
    return z


def test_noise_is_standard_normal(stream):
    x = np.sort(stream.reshape(-1))
    n = x.size
    cdf = norm_cdf(x)
    i = np.arange(1, n + 1)
    d = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    stats = {"KS": d * math.sqrt(n), "mean": abs(x.mean()) * math.sqrt(n), "var": abs((x ** 2).mean() - x.mean() ** 2 - 1) * math.sqrt(n / 2),
             "m4": abs((x ** 4).mean() - 3) * math.sqrt(n / 96)}
    print("[rng] " + ", ".join(f"{k} {v:.2f}" for k, v in stats.items()))
    assert stats["KS"] < 3.27, stats
    for k in ("mean", "var", "m4"):
        assert stats[k] < SIGMAS, (k, stats)


def test_noise_is_uncorrelated_inside_a_quad_and_along_the_stream(stream):
    z = stream
    stats = {"z0.z1": corr_z(z[:, 0], z[:, 1]), "z0.z2": corr_z(z[:, 0], z[:, 2]), "z1.z3": corr_z(z[:, 1], z[:, 3]),
             "z2.z3": corr_z(z[:, 2], z[:, 3]), "z0^2.z1^2": corr_z(z[:, 0] ** 2, z[:, 1] ** 2), "z2^2.z3^2": corr_z(z[:, 2] ** 2, z[:, 3] ** 2)}
    flat = z.reshape(-1)
    for lag in (1, 2, 3, 4, 5, 8, 263, 1024):
        stats[f"lag {lag}"] = corr_z(flat[:-lag], flat[lag:])
    print("[rng] " + ", ".join(f"{k} {v:+.2f}" for k, v in stats.items()))
    for k, v in stats.items():
        assert abs(v) < SIGMAS, (k, v)


def test_streams_of_other_keys_are_uncorrelated(stream):
    q = np.arange(65536, dtype=np.uint64)
    flat = stream.reshape(-1)
    for seed, sample, step in [(7, 1, 3), (7, 0, 4), (7, 0, 2), (8, 0, 3), (7, 0, 259), (7, 0, 65539), (7, 0, -1), (7 + (1 << 32), 0, 3), (7, 1 << 32, 3)]:
        _, other = R.normal_quads(seed, sample, step, q)
        v = corr_z(flat, other.reshape(-1))
        print(f"[rng] (7, 0, 3) x ({seed}, {sample}, {step}): {v:+.2f}")
        assert abs(v) < SIGMAS, (seed, sample, step, v)


def test_tail_counts_follow_the_normal_law():
    _, z = R.normal_quads(11, 5, 0, np.arange(1 << 20, dtype=np.uint64))
    a = np.abs(z.reshape(-1))
    for t in (3.0, 4.0, 4.5):
        want = a.size * math.erfc(t / math.sqrt(2.0))
        got = int((a > t).sum())
        print(f"[rng] |z| > {t}: {got} (expected {want:.1f})")
        assert abs(got - want) <= SIGMAS * math.sqrt(want), (t, got, want)


def test_layout_of_normals_matches_the_quads():
    """normals() = the [B, per_sample] layout of afm_randn: sample b is keyed by sample_index0 + b, a partial last quad is cut."""
    z32, z64 = R.normals(7, (1 << 32) - 1, 3, 2, 13)
    assert z32.shape == z64.shape == (2, 13) and z32.dtype == np.float32 and z64.dtype == np.float64
    for b in range(2):
        q32, q64 = R.normal_quads(7, (1 << 32) - 1 + b, 3, np.arange(4, dtype=np.uint64))
        assert np.array_equal(z64[b], q64.reshape(-1)[:13]) and np.array_equal(z32[b], q32.reshape(-1)[:13])
    assert np.abs(z32 - z64).max() < 4e-6                             # the float32 chain is the same function


# ------------------------------------------------------------------------------------------------ dropout keep-mask
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_mask_is_bernoulli_and_independent(p):
    rows, cols = 2048, 512
    m7, inv = R.keep_mask(p, 99, 7, rows, cols)
    m8, _ = R.keep_mask(p, 99, 8, rows, cols)
    assert m7.dtype == np.bool_ and m7.shape == (rows, cols)
    assert inv == np.float32(1.0) / (np.float32(1.0) - np.float32(p)) and abs(float(inv) - 1 / (1 - p)) < 1e-6 / (1 - p)
    n = rows * cols
    pf = float(np.float32(p))
    for name, m in (("id 7", m7), ("id 8", m8)):
        z = (m.mean() - (1 - pf)) / math.sqrt(pf * (1 - pf) / n)
        x = m.astype(np.float64)
        stats = {"keep": z, "row lag 1": corr_z(x[1:].reshape(-1), x[:-1].reshape(-1)), "col lag 1": corr_z(x[:, 1:].reshape(-1), x[:, :-1].reshape(-1))}
        rv, cv = x.sum(1).var(ddof=1) / (cols * pf * (1 - pf)), x.sum(0).var(ddof=1) / (rows * pf * (1 - pf))
        print(f"[mask] p {p} {name}: " + ", ".join(f"{k} {v:+.2f}" for k, v in stats.items()) + f", row-sum var ratio {rv:.2f}, col-sum {cv:.2f}")
        for k, v in stats.items():
            assert abs(v) < SIGMAS, (name, k, v)
        assert 0.75 <= rv <= 1.25 and 0.75 <= cv <= 1.25, (name, rv, cv)
    v = corr_z(m7.astype(np.float64).reshape(-1), m8.astype(np.float64).reshape(-1))
    print(f"[mask] p {p} id 7 x id 8: {v:+.2f}")
    assert abs(v) < SIGMAS


def test_keep_mask_threshold_at_the_ends_of_p():
    rows, cols = 2048, 512
    draws = R.drop_draws(99, 7, rows, cols)
    assert draws.max() < (1 << 32)
    thresh, inv = R.drop_threshold(2.0 ** -31)
    assert thresh == 2 and inv == np.float32(1.0)
    m, _ = R.keep_mask(2.0 ** -31, 99, 7, rows, cols)
    assert np.array_equal(m, draws >= 2) and (~m).sum() == (draws < 2).sum()
    thresh, inv = R.drop_threshold(0.99999994)                        # float32 1 - 2^-24: p * 2^32 = 4294967040, the saturation point
    assert thresh == 0xFFFFFFFF and inv == np.float32(2.0 ** 24)
    m, _ = R.keep_mask(0.99999994, 99, 7, rows, cols)
    assert np.array_equal(m, draws == 0xFFFFFFFF)
    assert R.drop_threshold(1.0 - 2.0 ** -23)[0] == (1 << 32) - 512    # the float32 below: not saturated
    assert R.drop_threshold(0.5)[0] == 1 << 31 and R.drop_threshold(0.0)[0] == 0
