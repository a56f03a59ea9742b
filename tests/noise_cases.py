"""The cases of the state-noise tests (hf_state_noise, csrc/initial_conditions.hip)
and a numpy restatement of what the entry point computes.

  draws       g = np.random.RandomState(seed).standard_normal(3 nx): the legacy
              polar method from word 0 of the stream (ic_cases' protocol without
              the mode draws); blocks g_n = g[0:nx], g_u = g[nx:2nx], g_E = g[2nx:3nx]
  zero mean   channel n only: d = g_n - m, m = (float64 sum of g_n) / nx, the sum
              in the kernel's order: lane l adds its cells l, l + 64, ... in
              ascending order from 0.0, then v[l] += v[l ^ o] for o = 32 .. 1
  arithmetic  out[ch] = in[ch] + f32(sigma[ch]) * f32(d): a float32 product, then
              a float32 add; sigma[ch] == 0: the row is copied
  plan        E is not perturbed (sigma_E must be 0) but recomputed from n':
              E[i] = f32(sum_j c[(i - j) mod nx] (n'[j] - 1)) in float64, c the
              circulant column of the spectral operator (plan[0:nx])

polar() states the draw protocol word by word (with its mutant, x1 and x2 of an
attempt swapped); tests/test_noise_cases_cpu.py shows it equal to numpy's
standard_normal, which reference() then uses.
"""
import math

import numpy as np

import ic_cases as C

NXS = C.NXS
SEEDS = C.SEEDS
SIGMAS = ((1e-2, 1e-2, 0.0), (0.0, 3e-3, 0.0), (1e-2, 0.0, 5e-3))
CASES = [(nx, sigma, zm) for nx in NXS for sigma in SIGMAS for zm in (True, False)]
COUNTS = (1, 2, 3, 51, 750, 18432)
MUTANTS = ("swap_x1_x2", "no_zero_mean", "blocks_u_n_E")


def polar(seed, count, swap=False):
    """standard_normal(count) from the raw word stream; swap: the mutant that
    yields f x1 first, then f x2."""
    cap = 2 * count + 256
    w = [int(v) for v in C.stream(seed, 4 * cap)]
    out, pos = [], 0
    for _ in range(cap):
        if len(out) >= count:
            break
        a, b, c, d = w[pos:pos + 4]
        pos += 4
        x1 = 2.0 * (((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0) - 1.0
        x2 = 2.0 * (((c >> 5) * 67108864.0 + (d >> 6)) / 9007199254740992.0) - 1.0
        r2 = x1 * x1 + x2 * x2
        if r2 >= 1.0 or r2 == 0.0:
            continue
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        out += [f * x1, f * x2] if swap else [f * x2, f * x1]
    assert len(out) >= count, "attempts exhausted"
    return np.asarray(out[:count])


_GAUSS = {}


def gauss(seed, count):
    """numpy's own standard_normal(count) for the seed, cached."""
    if (seed, count) not in _GAUSS:
        _GAUSS[seed, count] = np.random.RandomState(seed).standard_normal(count)
    return _GAUSS[seed, count]


def fixed_order_sum(g):
    """The kernel's float64 sum: per lane ascending, then the xor tree."""
    part = np.zeros(64)
    for k in range(0, g.size, 64):
        chunk = g[k:k + 64]
        part[:chunk.size] += chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ o]
    return part[0]


def reference(seed, nx, sigma, zero_mean, state, plan=None, mutant=None):
    """-> dict: out [3,nx] float32, noise [3,nx] float32 (the values added), d
    [3,nx] float64.  state [3,nx] float32; plan: None or the spectral plan
    (float64, at least nx long).  mutant: one of MUTANTS, a wrong restatement
    the tests must tell from the right one."""
    assert mutant in (None,) + MUTANTS
    state = np.asarray(state, dtype=np.float32)
    g = polar(seed, 3 * nx, swap=True) if mutant == "swap_x1_x2" else gauss(seed, 3 * nx)
    blocks = [g[0:nx], g[nx:2 * nx], g[2 * nx:3 * nx]]
    if mutant == "blocks_u_n_E":
        blocks = [blocks[1], blocks[0], blocks[2]]
    d = np.stack(blocks).astype(np.float64)
    if zero_mean and mutant != "no_zero_mean":
        d[0] = d[0] - fixed_order_sum(d[0]) / nx
    out, noise = state.copy(), np.zeros((3, nx), dtype=np.float32)
    for ch in range(3):
        s = np.float32(sigma[ch])
        if s == 0 or (ch == 2 and plan is not None):
            continue
        noise[ch] = s * d[ch].astype(np.float32)
        out[ch] = state[ch] + noise[ch]
    if plan is not None:
        assert sigma[2] == 0
        c = np.asarray(plan, dtype=np.float64)[:nx]
        idx = (np.arange(nx)[:, None] - np.arange(nx)[None, :]) % nx
        out[2] = (c[idx] @ (out[0].astype(np.float64) - 1.0)).astype(np.float32)
    return dict(out=out, noise=noise, d=d)


def states(nx, B=len(SEEDS)):
    """Smooth start states [B,3,nx] float32 of the solver's magnitudes (n near 1,
    u and E a few tenths), one per seed of the table."""
    x = (np.arange(nx) + 0.5) * (2 * np.pi / nx)
    b = np.arange(B)[:, None]
    n = 1.0 + 0.3 * np.sin((1 + b % 3) * x + 0.1 * b)
    u = 0.2 * np.cos((1 + b % 2) * x + 0.3 * b)
    E = 0.3 * np.cos((1 + b % 3) * x + 0.1 * b) / (1 + b % 3)
    return np.stack([n, u, E], axis=1).astype(np.float32)
