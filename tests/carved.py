"""Helpers of the kernel-level GPU tests (test_train_glue_gpu.py, test_train_rows_gpu.py): guard-banded allocations, the library
handle, and the rounding gate that is measured against torch's own fp32 error."""
import torch

from cobevt_amd import autograd as ag

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
U = 2.0 ** -24                       # fp32 unit roundoff
UB = 2.0 ** -8                       # bf16 unit roundoff (8 significant bits): one output rounding
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = 1, 2, 4          # csrc/common.hpp
GUARD = 256                          # elements: every carved tensor stays 16-byte aligned
_INT_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int64: torch.int64}
_INT_SENTINEL = 0x5A5A5A5A5A5A5A5A


class Carved(object):
    """n elements in the middle of a sentinel-filled allocation (NaN for float types; the carved region starts as the sentinel too)"""

    def __init__(self, n, dtype, dev, guard=GUARD, behind=0):
        self.n, self.guard = n, guard
        fill = _INT_SENTINEL if dtype == torch.int64 else float("nan")
        self.big = torch.full((guard + n + guard + behind,), fill, dtype=dtype, device=dev)
        self.t = self.big[guard:guard + n]
        self.sentinel = torch.full((1,), fill, dtype=dtype).view(_INT_VIEW[dtype]).item()

    def check(self, what, written=True):
        """both guard bands bit-identical to the sentinel; the carved region finite (written = True), still the sentinel (False) or
        free (None: scratch)"""
        bits = self.big.view(_INT_VIEW[self.big.dtype])
        g, n = self.guard, self.n
        assert bool((bits[:g] == self.sentinel).all()), what + ": wrote in front of the buffer"
        assert bool((bits[g + n:] == self.sentinel).all()), what + ": wrote behind the buffer"
        if written is None:
            return self.t
        if written:
            if self.big.dtype.is_floating_point:
                assert bool(torch.isfinite(self.t).all()), what + ": an element that the contract says is written is not finite"
        else:
            assert bool((bits[g:g + n] == self.sentinel).all()), what + ": wrote a buffer it must leave alone"
        return self.t


def _lib():
    return ag._L.load()


def _dev(dev, *ts):
    """device copies, to be held by the caller until its launch is enqueued (a temporary's block could be handed out again before)"""
    return [None if t is None else t.to(dev) for t in ts]


def _ok(rc, what):
    ag._L.check(rc, what)


def _int_map(rows, c, dtype, seed):
    """integer-valued (rows, C) in [-8, 8] with a distinct offset per channel (neighbouring 8-channel groups differ)"""
    g = torch.Generator().manual_seed(seed)
    off = (torch.arange(c) * 7) % 9 - 4
    return (torch.randint(-4, 5, (rows, c), generator=g) + off).to(dtype)


def carved_from(t, dev):
    """a guard-banded device copy of `t` (an output that the kernel adds into, or a zero-initialised one)"""
    c = Carved(t.numel(), t.dtype, dev)
    c.t.copy_(t.reshape(-1))
    return c


def rounding_gate(what, got, ref, tor, bf16=False, log=None):
    """The measured rounding gate.  got / tor: the kernel's and torch's fp32 (or bf16) result of the same operation on the same inputs,
    ref: float64 of it, all on the CPU.  Element by element (per channel for channel sums, per pixel for maps), |got - ref| may be at most
    max(4 x torch's own |tor - ref| of that element, 8 u max|ref|) (+ 2^-8 |ref| where the output is stored as bf16); the floor, taken
    over the tensor, covers an element that torch happens to hit exactly.
    -> (kernel max error, torch max error, worst error / gate); raises on a miss."""
    got, ref, tor = got.double().cpu(), ref.double().cpu(), tor.double().cpu()
    assert got.shape == ref.shape == tor.shape, "%s: shapes %s %s %s" % (what, tuple(got.shape), tuple(ref.shape), tuple(tor.shape))
    assert bool(torch.isfinite(got).all()), what + ": non-finite values"
    ek, et = (got - ref).abs(), torch.nan_to_num((tor - ref).abs(), nan=0.0, posinf=0.0)      # where torch has no number: the floor
    gate = torch.maximum(4.0 * et, torch.full_like(et, 8.0 * U * float(ref.abs().max()))).expand_as(ek)
    if bf16:
        gate = gate + UB * ref.abs()
    ratio = float((ek / gate.clamp_min(1e-300)).max()) if ek.numel() else 0.0
    line = "%s: kernel %.3e torch %.3e worst err/gate %.3f" % (what, float(ek.max()), float(et.max()), ratio)
    print(line)
    if log is not None:
        log.append((what, float(ek.max()), float(et.max()), ratio))
    bad = ek > gate
    assert not bool(bad.any()), "%s - %d elements over the gate, first at %s" % (line, int(bad.sum()), bad.nonzero()[0].tolist())
    return float(ek.max()), float(et.max()), ratio
