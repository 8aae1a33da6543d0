"""What helpers.grad_close_elements catches and helpers.grad_close does not (CPU, oracle only).

A gradient tensor of the tracer is not one population.  attr_grad holds colour columns (rms ~0.1) next to a density
column (rms ~60); the points_grad of a flat batch whose rays start inside the foam has a few elements in the millions
(the reference's phantom first-cell term) over a median near 2.  grad_close measures every
element against the rms of its whole tensor, and the call sites add a relative L2 norm below 1e-5 -- also a whole-tensor
scale.  This file builds gradients that are plainly wrong (the oracle's own, mutated), asserts that the whole-tensor
checks accept the ones listed in `_PASSES_TODAY` -- the reason for the per-element criterion, kept checkable -- and that
grad_close_elements, at the k the GPU tests use (helpers.element_k of the case's own reordering noise k0), rejects every
one of them while it accepts what is only a reordering: the rays in reverse order, and four threads.

What the whole-tensor checks let through on these cases, measured with the oracle alone (relative L2 in brackets):
  d3-flat   a whole ray's contribution missing from points_grad, rays 63 / 64 / 255 / 3999 (8.5e-6 / 1.3e-6 / 2.2e-6 /
            2.1e-6); every colour column of attr_grad times 1.001 (1.2e-6)
  d1-image  every colour column of attr_grad times 1.001 (6.9e-6)
  d2-flat   nothing of what is tried here (colour times 1.001: 3.9e-5)
and what they do catch, on all three: the elements of points_grad below rms/100 set to 0, negated or times 1.1 (d3-flat:
2.5e-4 / 5.1e-4 / 2.5e-5 -- three elements out of 6042 are above rms/100, the largest 2.7e6, which is not enough of a tail
to hide the rest behind), the density column times (1 + 2e-5) (2.0e-5), a ray missing from attr_grad or point_error.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

# (d, seed, image, quantiles, with_error): rows of the GPU matrices (tests/test_gpu_parity.py, tests/test_gpu_half.py)
_CASE_KEYS = {
    "d3-flat": (3, 23, False, True, True),
    "d1-image": (1, 21, True, True, False),
    "d2-flat": (2, 22, False, False, True),
}
_CASES = {}
_DROPPED = (63, 64, 255, -1)


def _case(foam_factory, name):
    if name not in _CASES:
        _CASES[name] = H.backward_case(foam_factory, *_CASE_KEYS[name])
    return _CASES[name]


def _tensors(c):
    return [k for k in H.GRAD_TENSORS if k in c["ref"]]


def _today(got, ref):
    ok, rel, worst = H.grad_close(got, ref)
    return ok and rel < 1e-5, rel


def _elements(c, key, got):
    return H.grad_close_elements(got, c["ref"][key], c["ref"][key + "_mag"], H.element_k(c["k0"]))


def _one_ray(c, r):
    """Ray r's own contribution to every gradient tensor: the oracle on that ray alone."""
    n = int(np.prod(c["rays"].shape[:-1]))
    flat = lambda x, w: None if x is None else np.asarray(x).reshape((n,) + w)[r:r + 1 if r != -1 else None]
    fm, q = c["fm"], c["q"]
    nq = 0 if q is None else q.shape[-1]
    args = (c["d"], fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    return O.trace_backward(*args, flat(c["rays"], (6,)), flat(np.broadcast_to(c["starts"], c["rays"].shape[:-1]), ()),
                            flat(c["fwd"]["rgba"], (4,)), flat(c["g"], (4,)), depth_quantiles=flat(q, (nq,)),
                            depth_indices=flat(c["fwd"].get("depth_indices"), (nq,)), depth_grad_in=flat(c["dg"], (nq,)),
                            ray_error=flat(c["err"], ()), num_threads=1)


def _small(ref):
    """The nonzero elements below rms/100 of their tensor (rms over the nonzero elements, as grad_close takes it)."""
    nz = ref[ref != 0].astype(np.float64)
    return (ref != 0) & (np.abs(ref) < np.sqrt(np.mean(nz ** 2)) / 100.0)


def _mutants(c):
    """name -> (tensor, mutated copy).  Every mutant changes at least one touched element of its tensor."""
    ref = c["ref"]
    out = {}
    pg, ag = ref["points_grad"], ref["attr_grad"]
    small = _small(pg)
    out["points: elements below rms/100 set to 0"] = ("points_grad", np.where(small, np.float32(0), pg))
    out["points: elements below rms/100 with the sign flipped"] = ("points_grad", np.where(small, -pg, pg))
    out["points: elements below rms/100 times 1.1"] = ("points_grad", np.where(small, pg * np.float32(1.1), pg))
    colour = ag.copy()
    colour[:, :-1] *= np.float32(1.001)
    out["attr: colour columns times 1.001"] = ("attr_grad", colour)
    dens = ag.copy()
    dens[:, -1] *= np.float32(1.0 + 2e-5)
    out["attr: density column times (1 + 2e-5)"] = ("attr_grad", dens)
    skipped = 0
    for r in _DROPPED:
        row = _one_ray(c, r)
        if not any(np.any(row[k] != 0) for k in _tensors(c)):
            skipped += 1        # a corner ray of the image misses the foam: dropping it changes nothing
            continue
        for k in _tensors(c):
            if np.any(row[k] != 0):
                out["%s: ray %d dropped" % (k, r)] = (k, ref[k] - row[k])
    assert skipped <= 1, skipped
    return out


# mutants the whole-tensor checks accept (grad_close and relative L2 < 1e-5), per case
_PASSES_TODAY = {
    "d3-flat": ["attr: colour columns times 1.001"] + ["points_grad: ray %d dropped" % r for r in _DROPPED],
    "d1-image": ["attr: colour columns times 1.001"],
    "d2-flat": [],
}


def test_the_populations_are_what_the_criterion_is_for(foam_factory):
    """The numbers DESIGN.md section 2 quotes: the heavy tail of the flat batch's point gradient, and colour against
    density in attr_grad."""
    pg = _case(foam_factory, "d3-flat")["ref"]["points_grad"]
    nz = np.abs(pg[pg != 0].astype(np.float64))
    rms = np.sqrt(np.mean(nz ** 2))
    big = int((nz >= rms / 100.0).sum())
    print("d3-flat points_grad: %d nonzero, rms %.3g, max %.3g, median %.3g, %d at or above rms/100"
          % (nz.size, rms, nz.max(), np.median(nz), big))
    assert nz.size > 5000 and big <= 12 and nz.max() > 1e5 * np.median(nz) and np.median(nz) < 100.0
    for name in ("d1-image", "d2-flat"):
        ag = _case(foam_factory, name)["ref"]["attr_grad"].astype(np.float64)
        r = lambda x: np.sqrt(np.mean(x[x != 0] ** 2))
        anz = np.abs(ag[ag != 0])
        print("%s attr_grad: density rms %.3g, colour rms %.3g, share of nonzero elements below 1e-3 rms %.2f, below "
              "rms/100 %.2f" % (name, r(ag[:, -1]), r(ag[:, :-1]), (anz < 1e-3 * r(ag)).mean(), (anz < r(ag) / 100).mean()))
        assert r(ag[:, -1]) > 50 * r(ag[:, :-1])
        assert (anz < r(ag) / 100).mean() > 0.4


@pytest.mark.parametrize("name", list(_CASE_KEYS))
def test_reorderings_are_accepted(foam_factory, name):
    """The oracle with the rays in reverse order (k0 itself: accepted by construction, with the factor of element_k to
    spare) and with four threads (partial sums per thread, merged with atomics in any order)."""
    c = _case(foam_factory, name)
    k = H.element_k(c["k0"])
    print(name, "k0 by tensor", c["k0_by_tensor"], "k", k)
    assert 1.0 <= c["k0"] <= 64.0 and k <= 256.0, c["k0_by_tensor"]
    fm = c["fm"]
    args = (c["d"], fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    four = O.trace_backward(*args, c["rays"], c["starts"], c["fwd"]["rgba"], c["g"], depth_quantiles=c["q"],
                            depth_indices=c["fwd"].get("depth_indices"), depth_grad_in=c["dg"], ray_error=c["err"],
                            num_threads=4)
    for key in _tensors(c):
        ok, worst, where = _elements(c, key, four[key])
        print(name, key, "four threads: worst ratio %.2f at %s" % (worst, where))
        assert ok, (key, worst, where)
        assert c["k0_by_tensor"][key] <= c["k0"]
        ok, worst, where = _elements(c, key, c["ref"][key])
        assert ok and worst == 0.0


@pytest.mark.parametrize("name", list(_CASE_KEYS))
def test_mutants_are_rejected_and_some_pass_the_whole_tensor_checks(foam_factory, name):
    c = _case(foam_factory, name)
    mutants = _mutants(c)
    assert all(m in mutants for m in _PASSES_TODAY[name]), sorted(mutants)
    wrong = []
    for what, (key, got) in mutants.items():
        ref, mag = c["ref"][key], c["ref"][key + "_mag"]
        assert np.any((got != ref) & (mag != 0)), what
        ok, worst, where = _elements(c, key, got)
        passes_today, rel = _today(got, ref)
        print("%s | %s | per element: %s (worst ratio %.3g at %s) | whole tensor: %s (rel L2 %.2g)"
              % (name, what, "accepted" if ok else "rejected", worst, where, "accepted" if passes_today else "rejected", rel))
        if ok:
            wrong.append(("accepted per element", what, worst, where))
        if what in _PASSES_TODAY[name] and not passes_today:
            wrong.append(("rejected by the whole-tensor checks", what, rel))
    assert not wrong, wrong


def test_an_untouched_element_must_be_zero(foam_factory):
    """mag == 0: no ray adds there, and anything but 0 is a write to the wrong row, however small."""
    c = _case(foam_factory, "d2-flat")
    for key in _tensors(c):
        ref, mag = c["ref"][key], c["ref"][key + "_mag"]
        idx = tuple(int(i) for i in np.argwhere(mag == 0)[0])
        got = ref.copy()
        got[idx] = np.float32(1e-30)
        ok, worst, where = _elements(c, key, got)
        assert not ok and worst == np.inf and where == idx, (key, worst, where)
        got[idx] = np.float32(-0.0)
        assert _elements(c, key, got)[0]


def test_fp16_outputs_get_one_rounding_and_no_more(foam_factory):
    """extra_rel = 2^-11 and extra_abs = 2^-25: the fp32 sums rounded to half once pass -- without the absolute term they
    do not, because a sum below 2^-14 lands among the subnormal halves, half a step of 2^-24 away whatever its size --
    and rounded to the next half up, a whole step from where they belong, they fail."""
    c = _case(foam_factory, "d2-flat")
    ref, mag = c["ref"]["attr_grad"], c["ref"]["attr_grad_mag"]
    assert np.any((ref != 0) & (np.abs(ref) < 2.0 ** -14))
    k = H.element_k(c["k0"])
    half = ref.astype(np.float16)
    once = dict(extra_rel=2.0 ** -11, extra_abs=2.0 ** -25)
    assert H.grad_close_elements(half, ref, mag, k, **once)[0]
    assert not H.grad_close_elements(half, ref, mag, k, extra_rel=2.0 ** -11)[0]
    assert not H.grad_close_elements(half, ref, mag, k)[0]
    up = np.nextafter(half, np.float16(np.inf))
    assert not H.grad_close_elements(np.where(np.abs(ref) >= 2.0 ** -14, up, half), ref, mag, k, **once)[0]
    assert not H.grad_close_elements(np.where(np.abs(ref) < 2.0 ** -14, up, half), ref, mag, k, **once)[0]
