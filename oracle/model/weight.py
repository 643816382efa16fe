"""TropicalWeight as rustfst computes it (tropical_weight.rs, semiring.rs): every step cast through f32."""
import numpy as np


# ---------------------------------------------------------------- TropicalWeight (tropical_weight.rs, semiring.rs)
F32, INF = np.float32, np.float32(np.inf)
KDELTA = F32(1.0 / 1024.0)


def times(a, b):  # tropical_weight.rs:60-70
    a, b = F32(a), F32(b)
    return a if a == INF else (b if b == INF else F32(a + b))


def divide(a, b):  # tropical_weight.rs:128-131: plain a - b
    with np.errstate(invalid="ignore"):
        return F32(F32(a) - F32(b))


def approx_eq(a, b):  # semiring.rs:159-168
    return bool(F32(a) <= F32(F32(b) + KDELTA) and F32(b) <= F32(F32(a) + KDELTA))


def is_zero(w):
    return approx_eq(w, INF)


def is_one(w):
    return approx_eq(w, 0.0)


def weighted(w):
    return not is_zero(w) and not is_one(w)


def plus(a, b):  # plus_assign: exact <
    return b if b < a else a


KSHORTESTDELTA = 1e-6


def quantize(v, delta):  # semiring.rs:132-145
    if np.isinf(v):
        return F32(v)
    return F32(F32(np.floor(F32(F32(F32(v) / F32(delta)) + F32(0.5)))) * F32(delta))


def wkey(w):  # exact tuple identity: the value, -0.0 == +0.0
    w = F32(w)
    return 0 if w == 0 else int(w.view(np.uint32))
