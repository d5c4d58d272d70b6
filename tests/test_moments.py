"""Fused one-pass statistics (ops.moments): host path, Chan combination, and (GPU) the HIP kernel."""
import math

import pytest
import torch

from cuda_mpi_reductions_amd.ops import combine_moments, fill_, moments, synthetic


def ref(x):
    xd = x.double()
    return xd.mean().item(), xd.var(unbiased=False).item(), xd.min().item(), xd.max().item()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 2, 7, 1000, 100_003])
def test_host_moments(dt, n):
    x = synthetic(n, dt, seed=n) * 5 - 2
    m = moments(x)
    mean, var, mn, mx = ref(x)
    assert m["count"] == n and m["min"] == mn and m["max"] == mx
    assert abs(m["mean"] - mean) <= 1e-12 * max(1, abs(mean))
    assert abs(m["var"] - var) <= 1e-9 * max(1e-12, var) + 1e-15


def test_shifted_variance_is_stable():
    # |mean| >> std: the naive Σx²/n - mean² loses every digit, the shifted form does not.
    x = synthetic(100_000, torch.float64) * 1e-3 + 1e9
    m = moments(x)
    assert abs(m["var"] - ref(x)[1]) <= 1e-6 * ref(x)[1]


def test_chan_combination_matches_whole():
    x = synthetic(10_000, torch.float64, seed=3)
    from cuda_mpi_reductions_amd.ops.moments import _raw
    a, b = _raw(x[:3333]), _raw(x[3333:])
    n, mean, m2, mn, mx = combine_moments(a, b)
    wm, wv, wmn, wmx = ref(x)
    assert n == 10_000 and abs(mean - wm) < 1e-12 and abs(m2 / n - wv) < 1e-12 and mn == wmn and mx == wmx


def test_rejects_ints():
    with pytest.raises(TypeError):
        moments(torch.arange(10))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [1, 3, 63, 65, 4097, 1_000_003, (1 << 24) + 5])
def test_device_moments(dt, n):
    x = torch.empty(n, dtype=dt, device="cuda")
    fill_(x, "uniform", seed=n)
    x.mul_(7).sub_(3)
    m = moments(x)
    mean, var, mn, mx = ref(x)
    assert m["count"] == n and m["min"] == mn and m["max"] == mx
    assert abs(m["mean"] - mean) <= 1e-9 * max(1.0, abs(mean))
    assert abs(m["var"] - var) <= 1e-9 * max(1e-9, var)


# |mean| >> std on the device: x = c + k * s with integer k, exact in the dtype, so that every x - K of
# the shifted algorithm and both of its fp64 sums are exact and the file's own bounds hold as they are.
# |c| / s is 2^10 for the 16-bit types and 2^20 or more for fp32 / fp64. k is drawn from -8..8; bfloat16
# has 8 significant bits, so there only k in {-8, 0, 8} is a bfloat16 number next to c = 2^10 * s.
SHIFTED = {torch.float64: (2.0 ** 30, 2.0 ** -10, 1), torch.float32: (4096.0, 2.0 ** -8, 1),
           torch.float16: (1024.0, 1.0, 1), torch.bfloat16: (1024.0, 1.0, 8)}


def _shifted_case(dt, n):
    """(x, exact mean, exact population variance): the moments of k in integer arithmetic."""
    c, s, step = SHIFTED[dt]
    g = torch.Generator().manual_seed(n)
    k = (torch.randint(-8 // step, 8 // step + 1, (n,), generator=g) * step)
    k[0] = step  # an ordinary element as the shift
    x = (c + k.double() * s).to(dt)
    assert torch.equal(x.double(), c + k.double() * s) and abs(c) / s >= (2 ** 10 if dt.itemsize == 2 else 2 ** 20)
    s1, s2 = int(k.sum()), int((k * k).sum())
    return x, c + s * s1 / n, s * s * (n * s2 - s1 * s1) / (n * n)


def test_naive_variance_misses_the_bound_the_shifted_one_keeps():
    """Σx²/n - mean² in fp64, the arithmetic of the kernel without its shift, on the fp64 case: it misses
    the 1e-9 bound that test_device_shifted_variance asserts, so that test tells the two apart. The host
    path of moments() (the same shifted formula) keeps it."""
    x, mean, var = _shifted_case(torch.float64, 4097)
    naive = (x * x).sum().item() / x.numel() - (x.sum().item() / x.numel()) ** 2
    print(f"exact var {var!r} naive {naive!r}")
    assert abs(naive - var) > 1e-9 * max(1e-9, var)
    m = moments(x)
    assert abs(m["var"] - var) <= 1e-9 * max(1e-9, var) and abs(m["mean"] - mean) <= 1e-12 * max(1.0, abs(mean))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [4097, 1_000_003])
def test_device_shifted_variance(dt, n):
    x, mean, var = _shifted_case(dt, n)
    m = moments(x.cuda())
    assert m["count"] == n and m["min"] == x.double().min().item() and m["max"] == x.double().max().item()
    assert abs(m["mean"] - mean) <= 1e-12 * max(1.0, abs(mean)), (m["mean"], mean)
    assert abs(m["var"] - var) <= 1e-9 * max(1e-9, var), (m["var"], var)


@pytest.mark.gpu
def test_device_moments_misaligned_view():
    base = torch.empty(100_001, dtype=torch.float32, device="cuda")
    fill_(base, "uniform", seed=1)
    x = base[1:]
    m = moments(x)
    assert m["min"] == x.min().item() and abs(m["mean"] - x.double().mean().item()) < 1e-9
