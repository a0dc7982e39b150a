"""Float64 reference of one Adam / AdamW step with a per-element half-width for each of p, m and v, in the manner of
rows_bounds_ref.py: the kernel of csrc/train_glue.hip (cobevt_adam_prepare + cobevt_multi_adam) and torch.optim.Adam / AdamW in fp32
must both land inside [reference - e, reference + e] when started from the same stored fp32 values.

The step, in exact arithmetic, from fp32 inputs (p, g, m, v), the step count t (already advanced) and fp64 hyper-parameters:

    DECAY = 1 - lr wd   STEP = lr / (1 - beta1^t)   RBC2 = 1 / sqrt(1 - beta2^t)   INV = 1 / grad_scale (1 without a scale)
    G  = g INV                     (+ wd p in Adam mode)
    P1 = p DECAY                   (AdamW mode; P1 = p in Adam mode)
    M' = m + (G - m)(1 - beta1)
    V' = beta2 v + (1 - beta2) G G
    D  = sqrt(V') RBC2 + eps
    P' = P1 - STEP (M' / D)

How the half-widths are derived.  U = 2^-23: every fp32 operation of the kernel's sequence (one per line in adam_update) returns
its exact result with a relative error of at most U (round to nearest gives U / 2; the factor of two is the whole slack, and it
also covers a 1-ulp square root, torch's division by sqrt(bc2) in place of the multiplication by RBC2 and either association of
(1 - beta2) g g), plus T = 2^-149 absolute for a result in the subnormal range.  Every coefficient that reaches the kernel as an
fp32 number (DECAY or wd, STEP, RBC2, INV, 1 - beta1, beta2, 1 - beta2, eps) was rounded once from fp64: one U each, relative.
Writing x~ for a computed value, X for its exact counterpart and e_x >= |x~ - X|:

    product with a rounded coefficient C:  y~ = fl(c~ x~),  |c~ - C| <= U |C|
        e_in = |C| e_x + U |C| (|X| + e_x)  [operand and coefficient],  e_y = e_in + U (|C X| + e_in) + T  [this rounding]
    sum / difference:  e_y = e_a + e_b + U (|A +- B| + e_a + e_b) + T
        - the lerp's subtraction G - m is rounded against |G - m|, not against |G| + |m|: that is what keeps e_m at a few U |M'|
    product of two computed values:  e_y = |A| e_b + |B| e_a + e_a e_b + U (|A B| + that) + T
    square root:  |sqrt(v~) - sqrt(V')| <= e_v / (2 sqrt(V' - e_v)) where V' > e_v (the derivative at the lower end), and never more
        than sqrt(e_v) (|sqrt a - sqrt b| <= sqrt |a - b|); then its own rounding
    quotient:  |m~ / d~ - M' / D| <= (e_m + |M' / D| e_d) / (D - e_d)  (against the lower end of d; D - e_d > 0 is asserted), then
        its own rounding

No constant here is fitted to any implementation.  On p the half-width comes to about 3 U |p| (decay product, its coefficient, the
final subtraction) plus a few U of the update, while the weight-decay term itself is lr wd |p| - about five times that at the
reference's lr 2e-4, wd 1e-2 - so a missing or misplaced decay leaves the interval.

`emulate` is the kernel's sequence in numpy fp32 (one rounded operation per line), with the deliberate faults tests/test_optim.py
plants in it.
"""
import math

import numpy as np

U = 2.0 ** -23
T = 2.0 ** -149
FAULTS = ("no_weight_decay", "l2_in_adamw", "eps_inside_sqrt", "bc2_without_sqrt", "step_not_advanced", "inv_scale_ignored")


def coefficients(step, lr, beta1, beta2, weight_decay, adamw, grad_scale=None):
    """-> fp64 (decay | wd, step_size, rbc2, inv_scale) for the ADVANCED step count"""
    t = float(step)
    return (1.0 - lr * weight_decay if adamw else weight_decay, lr / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t),
            1.0 if grad_scale is None else 1.0 / float(grad_scale))


def _coef_mul(c, x, ex):
    """half-width of fl(c~ x~), c~ the fp32 rounding of the fp64 coefficient c"""
    c = abs(c)
    e_in = c * ex + U * c * (np.abs(x) + ex)
    return e_in + U * (c * np.abs(x) + e_in) + T


def _add(s, ea, eb):
    """fl(a~ +- b~) with exact result s"""
    return ea + eb + U * (np.abs(s) + ea + eb) + T


def _mul(a, ea, b, eb):
    e_in = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return e_in + U * (np.abs(a * b) + e_in) + T


def step_bounds(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, adamw=True, grad_scale=None):
    """One step from the stored fp32 arrays (any shape) and the ADVANCED step count `step` (= stored step + 1).
    -> (P, M, V, e_p, e_m, e_v): float64 exact results and half-widths."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    decay, step_size, rbc2, inv = coefficients(step, lr, beta1, beta2, weight_decay, adamw, grad_scale)
    zero = np.zeros_like(p)
    # g = g inv_scale
    G = g * inv
    e_g = zero if grad_scale is None else _coef_mul(inv, g, zero)          # (a product with 1 is exact)
    if adamw:
        P1 = p * decay
        e_p1 = _coef_mul(decay, p, zero)
    else:
        L2 = weight_decay * p
        e_l2 = _coef_mul(weight_decay, p, zero)
        e_g = _add(G + L2, e_g, e_l2)
        G = G + L2
        P1, e_p1 = p, zero
    # m = m + (g - m)(1 - beta1)
    DM = G - m
    e_dm = _add(DM, e_g, zero)
    TM = DM * (1.0 - beta1)
    e_tm = _coef_mul(1.0 - beta1, DM, e_dm)
    M = m + TM
    e_m = _add(M, zero, e_tm)
    # v = beta2 v + ((1 - beta2) g) g
    A = beta2 * v
    e_a = _coef_mul(beta2, v, zero)
    B = (1.0 - beta2) * G
    e_b = _coef_mul(1.0 - beta2, G, e_g)
    C = B * G
    e_c = _mul(B, e_b, G, e_g)
    V = A + C
    e_v = _add(V, e_a, e_c)
    # d = sqrt(v) rbc2 + eps
    S = np.sqrt(V)
    lower = np.maximum(V - e_v, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(lower > 0.0, e_v / (2.0 * np.sqrt(np.where(lower > 0.0, lower, 1.0))), np.inf)
    e_s = np.minimum(e_s, np.sqrt(e_v))
    e_s = e_s + U * (S + e_s) + T
    R = S * rbc2
    e_r = _coef_mul(rbc2, S, e_s)
    D = R + eps
    e_d = _add(D, e_r, U * eps * np.ones_like(p))
    assert np.all(D - e_d > 0.0), "optim_ref: the denominator's interval reaches zero (eps = 0 with a zero second moment?)"
    # p = p - step_size (m / d)
    Q = M / D
    e_q = (e_m + np.abs(Q) * e_d) / (D - e_d)
    e_q = e_q + U * (np.abs(Q) + e_q) + T
    UPD = step_size * Q
    e_u = _coef_mul(step_size, Q, e_q)
    P = P1 - UPD
    e_p = _add(P, e_p1, e_u)
    return P, M, V, e_p, e_m, e_v


def used(got, want, e):
    """max |got - want| / e over the elements (0 / 0 counts as 0: an exact result with a zero half-width)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / e)
    return float(r.max()) if r.size else 0.0


def outside(got, want, e):
    """boolean mask of the elements outside [want - e, want + e]"""
    return np.abs(np.asarray(got, dtype=np.float64) - want) > e


def emulate(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, adamw=True, grad_scale=None, fault=None):
    """The kernel's sequence in numpy fp32 from the STORED step count `step` (advanced here, as cobevt_adam_prepare does).
    -> (p, m, v) fp32.  fault: one of FAULTS, or None for the kernel as built."""
    assert fault is None or fault in FAULTS
    f = np.float32
    t = step if fault == "step_not_advanced" else step + 1
    decay, step_size, rbc2, inv = coefficients(t, lr, beta1, beta2, weight_decay, adamw, grad_scale)
    if fault == "bc2_without_sqrt":
        rbc2 = 1.0 / (1.0 - beta2 ** float(t))
    if fault == "inv_scale_ignored":
        inv = 1.0
    if fault == "no_weight_decay":
        decay = 1.0 if adamw else 0.0
    c0, c1, c2, c3 = f(decay), f(step_size), f(rbc2), f(inv)
    omb1, b2, omb2, epsf = f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps)
    p, g, m, v = (np.array(x, dtype=np.float32) for x in (p, g, m, v))
    g = g * c3
    if not adamw:
        l2 = c0 * p
        g = g + l2
    elif fault == "l2_in_adamw":
        l2 = f(weight_decay) * p
        g = g + l2
    else:
        p = p * c0
    dm = g - m
    tm = dm * omb1
    m = m + tm
    a = b2 * v
    b = omb2 * g
    gg = b * g
    v = a + gg
    if fault == "eps_inside_sqrt":
        s = np.sqrt(v + epsf)
        d = s * c2
    else:
        s = np.sqrt(v)
        r = s * c2
        d = r + epsf
    q = m / d
    u = c1 * q
    p = p - u
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v
