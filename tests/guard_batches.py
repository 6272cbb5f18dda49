"""Test infrastructure: input batches whose rows drive every branch of the unbiased kernels'
x / den (div_plan / div4) and of the sign / zero handling, shared by the GPU tests."""
import numpy as np

f32 = np.float32


def division_guard_batch(n, d, rng, extras=False):
    """Rows that drive every branch of the kernels' x / den (div_plan / div4): ordinary
    rows (fast path), rows with tiny, subnormal, huge and non-finite elements (per-element
    IEEE fallback), zero-heavy rows (zeros stay on the fast path), a row with L1 >= 2^40
    (whole client on the IEEE division), an all-zero row (den = 1e-12) and rows whose
    quotients all fall under the guard threshold.

    extras (drawn after the rows above, which stay as they are): -0.0 and tiny negative
    coordinates (normal and subnormal) in the ordinary rows, whose sign must survive a zero
    count, and one heavy-tailed row (Cauchy: a few coordinates carry most of the L1)."""
    x = rng.standard_normal((n, d)).astype(f32)
    for j in range(n):
        kind = j % 8
        idx = rng.integers(0, d, size=max(1, d // 64))
        if kind == 1:
            x[j, idx] *= np.float32(1e-40)                        # subnormal elements
        elif kind == 2:
            x[j, idx] = (rng.standard_normal(idx.size) * 1e-25).astype(f32)   # tiny normals
        elif kind == 3:
            x[j] *= np.float32(1e10)                              # L1 >= 2^40: IEEE path per client
        elif kind == 4:
            x[j, rng.random(d) < 0.9] = 0.0                       # sparse: zeros on the fast path
        elif kind == 5:
            x[j] *= np.float32(1e-30)                             # every quotient under the threshold
        elif kind == 6:
            x[j, idx[:3]] = [np.inf, -np.inf, np.nan][: min(3, idx.size)]
        elif kind == 7:
            x[j, idx] *= np.float32(1e30)                         # huge elements, q still finite
    x[n // 2] = 0.0                                               # den = 1e-12 exactly
    if extras:
        for j in range(0, n, 8):
            if j == n // 2:
                continue
            idx = rng.integers(0, d, size=max(3, d // 32))
            x[j, idx[0::3]] = f32(-0.0)
            x[j, idx[1::3]] = -np.abs(rng.standard_normal(idx[1::3].size) * 1e-30).astype(f32)
            x[j, idx[2::3]] = f32(-1e-42)                         # negative subnormal
        if n > 8 and n // 2 != 8:
            x[8] =rng.standard_cauchy(d).astype(f32)
    return x


def guard_draws(n, rng):
    """Per-client X in [0, 1) with both ends of the range: 0 and the largest f32 below 1."""
    X = rng.random(n).astype(f32)
    X[0] = f32(0.0)
    if n > 1:
        X[1] = np.nextafter(f32(1.0), f32(0.0))
    return X
