"""The assertions of tests/test_step_tail_gpu.py must be able to fail: on the CPU, the fp32 emulation of the kernels passes them on
every case the GPU tests run, tests.util.TorchStepKernels (the stand-in the gloo tests inject) passes them too, and every listed
mutant of the emulation is rejected on the same inputs."""
import math

import pytest
import torch

from tests import step_tail_ref as R
from tests.util import TorchStepKernels


def _worst_over(impl, sizes, K=None):
    worst = dict(m=0.0, v=0.0, p=0.0)
    for n in sizes:
        for case in R.adam_cases(n):
            r = R.run_adam_case(impl, case, K=K)
            worst = {k: max(worst[k], r[k]) for k in worst}
    return worst


def test_adam_bound_constants():
    """ADAM_K is 4 x the emulation's worst ratio to each bound shape over every case, rounded up to a power of two -- derived
    from the emulation, not fitted to the kernel (measured here: m 2.178, v 4.066, p 4.629 -> 16, 32, 32).  The random inputs
    come from vectorised library routines whose last bit may differ between CPUs and the ratio is a maximum over millions of
    elements, so the derivation is asserted as the interval the rounding allows, 4 x ratio <= K < 8 x ratio, widened to 16 x."""
    worst = _worst_over(R.adam_emulation, R.ADAM_SIZES)
    print("adam emulation worst ratios: m %.3f v %.3f p %.3f" % (worst["m"], worst["v"], worst["p"]))
    for k in "mvp":
        assert 4.0 * worst[k] <= R.ADAM_K[k] < 16.0 * worst[k], (k, worst[k], R.ADAM_K[k])
        assert R.ADAM_K[k] == 2.0 ** round(math.log2(R.ADAM_K[k]))


def test_adam_cases_cover_what_the_issue_lists():
    cases = [c for n in R.ADAM_SIZES for c in R.adam_cases(n)]
    for n in R.ADAM_SIZES:
        mine = [c for c in cases if c["n"] == n]
        assert {c["off"] for c in mine} == set(R.ADAM_OFFSETS)
        assert {c["step"] for c in mine} == set(R.ADAM_STEPS)
        assert {c["gscale"] for c in mine} == set(R.ADAM_GSCALES)
        assert {(c["max_norm"], c["gnorm"], c["zero_grad"]) for c in mine} == set(R.ADAM_CLIPS)
    # the clip settings really are on both sides of max_norm, for both scales
    for gs in R.ADAM_GSCALES:
        assert R.CLIP / (16.0 * gs + 1e-6) < 0.5 and R.CLIP / (0.1 * gs + 1e-6) > 2.0
    p, g, m, v = R.adam_buffers(cases[200])
    assert float(m.nan_to_num().abs().max()) > 0 and float(v.nan_to_num().abs().max()) > 0


def _torch_step_kernels(P, G, M, V, off, n, lr, b1, b2, eps, gnorm, max_norm, gscale, step):
    TorchStepKernels().adam(P[off:off + n], G[off:off + n], M[off:off + n], V[off:off + n], lr, b1, b2, eps, gnorm, max_norm, gscale,
                            step)


def test_torch_step_kernels_agree_with_float64():
    """The stand-in of the gloo tests means what the kernel means: same bounds, same cases."""
    worst = _worst_over(_torch_step_kernels, R.ADAM_SIZES)
    print("TorchStepKernels worst ratios: m %.3f v %.3f p %.3f" % (worst["m"], worst["v"], worst["p"]))


@pytest.mark.parametrize("mutant", R.ADAM_MUTANTS)
def test_adam_mutant_is_rejected(mutant):
    impl = lambda *a: R.adam_emulation(*a, mutant=mutant)
    rejected = 0
    for n in R.ADAM_SIZES[:-1]:
        for case in R.adam_cases(n):
            try:
                R.run_adam_case(impl, case)
            except AssertionError:
                rejected += 1
    print("%s: rejected on %d cases" % (mutant, rejected))
    assert rejected > 0, mutant


def test_l2_one_ulp_check_can_fail():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    ok, ref = R.l2_within_one_ulp(torch.tensor(ref_f32(g)), g)
    assert ok
    assert not R.l2_within_one_ulp(torch.tensor(ref_f32(g) * (1 + 3 * 2.0 ** -23)), g)[0]
    assert not R.l2_within_one_ulp(g.norm() * 0.0, g)[0]
    # an fp32 sum of squares overflows / underflows where the double sum does not
    for mag in (1e20, 1e-30):
        big = torch.full((257,), mag)
        assert R.l2_within_one_ulp(torch.tensor(ref_f32(big)), big)[0]
        assert not R.l2_within_one_ulp(torch.sqrt((big * big).sum()), big)[0]


def ref_f32(g):
    import numpy as np
    return float(np.float32(R.l2norm64(g)))


# ---- gather -------------------------------------------------------------------------------------------------------------------
def _gather_passes(mutant):
    ok = True
    for count, zero_edges in R.gather_cases():
        entries, dst0 = R.gather_case(count, zero_edges)
        dst = dst0.clone()
        R.gather_emulation(dst, entries, mutant=mutant)
        ok = ok and R.same_bits(dst, R.gather_expected(dst0, entries))
    return ok


def test_gather_emulation_passes_and_cases_have_the_edges():
    assert _gather_passes(None)
    for count, zero_edges in R.gather_cases():
        entries, dst0 = R.gather_case(count, zero_edges)
        assert len(entries) == count
        if count >= 5:
            assert any(s is None and n > 0 for s, _, n in entries)
            assert any(s is not None and s.storage_offset() == 1 and n >= 4 for s, _, n in entries)
            assert any(o % 4 for _, o, _ in entries)
            if zero_edges:
                ns = [n for _, _, n in entries]
                assert ns[0] == 0 and ns[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(ns[1:-1], ns[2:-1]))
        covered = torch.zeros(dst0.numel(), dtype=torch.bool)
        for _, o, n in entries:
            assert not bool(covered[o:o + n].any())
            covered[o:o + n] = True
        assert not bool(covered.all())            # canaries between and around the entries


@pytest.mark.parametrize("mutant", R.GATHER_MUTANTS)
def test_gather_mutant_is_rejected(mutant):
    assert not _gather_passes(mutant)


# ---- reduction ----------------------------------------------------------------------------------------------------------------
def test_reduce_emulation_passes():
    worst = max(R.run_reduce_case(R.reduce_emulation, c) for c in R.reduce_cases())
    print("reduce emulation worst ratio to S u sum|partial|: %.3f" % worst)


@pytest.mark.parametrize("mutant", R.REDUCE_MUTANTS)
def test_reduce_mutant_is_rejected(mutant):
    impl = lambda *a: R.reduce_emulation(*a, mutant=mutant)
    rejected = 0
    for c in R.reduce_cases():
        try:
            R.run_reduce_case(impl, c)
        except AssertionError:
            rejected += 1
    print("%s: rejected on %d cases" % (mutant, rejected))
    assert rejected > 0


def test_reduce_vec_is_overwritten_not_accumulated_in_the_reference():
    """beta = 1 cases carry a non-zero prior vec: an implementation that accumulated into it would leave the bound."""
    case = next(c for c in R.reduce_cases() if c[5] and c[7] == 1.0 and c[0] == 5)

    def accumulating(case, partial, C, vec):
        old = vec.clone()
        R.reduce_emulation(case, partial, C, vec)
        vec.add_(old)
    with pytest.raises(AssertionError):
        R.run_reduce_case(accumulating, case)
