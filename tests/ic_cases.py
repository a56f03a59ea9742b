"""The (seed, nx) cases of the device initial-condition generator's tests, and
a pure-Python replay of its draw protocol over the raw MT19937 word stream.

The generator (hf_initial_conditions, csrc/initial_conditions.hip) must consume
the 32-bit words np.random.RandomState(seed) consumes in
BaselineSolver._modes (src/baseline_solver.py:29-51).  The replay here states
that protocol in plain Python, word by word, over
RandomState(seed).randint(0, 1 << 32, dtype=np.uint32) (one word per value);
tests/test_ic_cases_cpu.py shows it equal to numpy's own draws and to _modes bit
for bit, so what the GPU tests expect is numpy's, and the replay says which
paths each case takes (rejected tries, 624-word blocks crossed).

  randint(lo, hi)  rng = hi-1-lo, mask = smallest 2^k-1 >= rng; v = word & mask
                   per try, accepted when v <= rng
  rand()           (a 2^26 + b) / 2^53, a = word >> 5, b = next word >> 6
  randn(nx)        polar: x1 = 2 rand() - 1, x2 = 2 rand() - 1, r2 = x1 x1 + x2 x2,
                   rejected when r2 >= 1 or r2 == 0; f = sqrt(-2 log(r2) / r2);
                   f x2 first, then f x1; four words per attempt
  order            k = randint(3, 6); k x (km = randint(1, 6), amp = 0.15 + 0.15
                   rand(), ph = 2 pi rand()); 2 x (km, amp = 0.1 + 0.1 rand(),
                   ph); randn(nx)
  arithmetic       n = f32 1; n += f32(amp) * f32(sin(km x + ph)) per mode (the
                   argument and sin in float64, product and sum in float32); u
                   likewise from 0 with cos; u += f32(0.05) * f32(gauss)
"""
import math

import numpy as np

TABLE_LEN = 23     # HF_IC_TABLE_LEN: k, 7 x (km, amp, ph), words
N_SLOTS, U_SLOT0 = 7, 5
NXS = (16, 17, 64, 250, 256, 1024)
# edge seeds, a run of ordinary ones, and one seed twice (rows must not depend on position)
SEEDS = (0, 1, 42, 2 ** 32 - 1) + tuple(range(1000, 1016)) + (42,)
CASES = [(s, nx) for nx in NXS for s in SEEDS]
BLOCK = 624


def stream(seed, count):
    return np.random.RandomState(seed).randint(0, 1 << 32, size=count, dtype=np.uint32)


def stream_bound(nx):
    """More words than any replay of nx cells reads: 8 randint x 64 tries, 28
    words of rand, 2 nx + 256 gauss attempts of four (the kernel's bounds)."""
    return 8 * 64 + 28 + 4 * (2 * nx + 256)


class Replay:
    def __init__(self, seed, nx):
        self.w = [int(v) for v in stream(seed, stream_bound(nx))]
        self.pos = 0
        self.randint_rejects = 0
        self.gauss_rejects = 0

    def word(self):
        self.pos += 1
        return self.w[self.pos - 1]

    def randint(self, lo, hi):
        rng = hi - 1 - lo
        mask = (1 << rng.bit_length()) - 1
        for _ in range(64):
            v = self.word() & mask
            if v <= rng:
                return lo + v
            self.randint_rejects += 1
        raise AssertionError("randint: 64 tries rejected")

    def rand(self):
        a = self.word() >> 5
        b = self.word() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def randn(self, nx):
        out = []
        for _ in range(2 * nx + 256):
            if len(out) >= nx:
                break
            x1 = 2.0 * self.rand() - 1.0
            x2 = 2.0 * self.rand() - 1.0
            r2 = x1 * x1 + x2 * x2
            if r2 >= 1.0 or r2 == 0.0:
                self.gauss_rejects += 1
                continue
            f = math.sqrt(-2.0 * math.log(r2) / r2)
            out += [f * x2, f * x1]
        assert len(out) >= nx, "randn: attempts exhausted"
        return np.asarray(out[:nx])     # odd nx: the cached second value is dropped


def replay(seed, nx):
    """-> dict: table [TABLE_LEN] float64 in HF_IC_TABLE_LEN's layout, gauss [nx]
    float64, words, mode_words, randint_rejects, gauss_rejects."""
    r = Replay(seed, nx)
    t = np.zeros(TABLE_LEN)
    k = r.randint(3, 6)
    t[0] = k
    for slot in list(range(k)) + [U_SLOT0, U_SLOT0 + 1]:
        a = 0.15 if slot < U_SLOT0 else 0.1
        km = r.randint(1, 6)
        amp = a + a * r.rand()
        ph = 2 * np.pi * r.rand()
        t[1 + 3 * slot:4 + 3 * slot] = (km, amp, ph)
    mode_words = r.pos
    gauss = r.randn(nx)
    t[TABLE_LEN - 1] = r.pos
    return dict(table=t, gauss=gauss, words=r.pos, mode_words=mode_words, randint_rejects=r.randint_rejects,
                gauss_rejects=r.gauss_rejects)


def fields(table, gauss, x):
    """n, u (float32) from a draw table and gauss, in _modes' arithmetic."""
    n = np.full(x.size, 1.0, dtype=np.float32)
    for slot in range(int(table[0])):
        km, amp, ph = table[1 + 3 * slot:4 + 3 * slot]
        n += np.float32(amp) * np.sin(km * x + ph).astype(np.float32)
    u = np.zeros(x.size, dtype=np.float32)
    for slot in (U_SLOT0, U_SLOT0 + 1):
        km, amp, ph = table[1 + 3 * slot:4 + 3 * slot]
        u += np.float32(amp) * np.cos(km * x + ph).astype(np.float32)
    u += np.float32(0.05) * gauss.astype(np.float32)
    return n, u


def numpy_draws(seed, nx):
    """numpy's own draws in _modes' order -> (table without the word count,
    randn(nx), the four words numpy draws next: they locate the end of the
    consumed stream)."""
    rs = np.random.RandomState(seed)
    t = np.zeros(TABLE_LEN)
    k = rs.randint(3, 6)
    t[0] = k
    for slot in list(range(k)) + [U_SLOT0, U_SLOT0 + 1]:
        a = 0.15 if slot < U_SLOT0 else 0.1
        t[1 + 3 * slot:4 + 3 * slot] = (rs.randint(1, 6), a + a * rs.rand(), 2 * np.pi * rs.rand())
    gauss = rs.randn(nx)
    return t, gauss, rs.randint(0, 1 << 32, size=4, dtype=np.uint32)


_EXPECTED = {}


def expected_table(seed, nx):
    """numpy's draws with the replay's word count (shown to be numpy's by
    tests/test_ic_cases_cpu.py), cached."""
    if (seed, nx) not in _EXPECTED:
        t, _, _ = numpy_draws(seed, nx)
        t[TABLE_LEN - 1] = replay(seed, nx)["words"]
        _EXPECTED[seed, nx] = t
    return _EXPECTED[seed, nx]
