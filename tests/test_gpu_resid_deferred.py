"""The two row passes of a block with the first one's residual store deferred
(vggt_resid_add_layernorm_nostore + vggt_resid_add2_layernorm) against the two
stored passes (vggt_resid_add_layernorm twice): bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


@pytest.mark.parametrize("next_norm", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("C", [256, 1024])
@pytest.mark.parametrize("M", [300, 1030])
def test_deferred_passes_bitwise_equal_stored_passes(N, M, C, mirror, next_norm):
    g = torch.Generator().manual_seed(M + C)
    dev = "cuda"
    x0 = torch.randn(M, C, generator=g).to(dev)
    pj = torch.randn(M, C, generator=g).to(torch.bfloat16).to(dev)
    f2 = torch.randn(M, C, generator=g).to(torch.bfloat16).to(dev)
    g1 = (0.5 + torch.rand(C, generator=g)).to(dev)
    g2 = (0.5 + torch.rand(C, generator=g)).to(dev)
    w2, b2 = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    w1, b1 = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    eps = 1e-6

    def outs():
        # the mirror is a strided view (one half of a concat buffer), as in the aggregator
        cat = torch.zeros(M, 2 * C, device=dev) if mirror else None
        return (x0.clone(), torch.zeros(M, C, device=dev, dtype=torch.bfloat16), cat,
                torch.zeros(M, C, device=dev, dtype=torch.bfloat16) if next_norm else None)

    xa, xn2a, cata, xn1a = outs()
    N.resid_add_layernorm(xa, pj, g1, None, w2, b2, eps, xn2a)
    N.resid_add_layernorm(xa, f2, g2, cata[:, C:] if mirror else None, w1 if next_norm else None,
                          b1 if next_norm else None, eps, xn1a)
    xb, xn2b, catb, xn1b = outs()
    N.resid_add_layernorm_nostore(xb, pj, g1, w2, b2, eps, xn2b)
    torch.cuda.synchronize()
    assert torch.equal(xb, x0)  # the first pass leaves x alone
    N.resid_add2_layernorm(xb, pj, g1, f2, g2, catb[:, C:] if mirror else None, w1 if next_norm else None,
                           b1 if next_norm else None, eps, xn1b)
    torch.cuda.synchronize()
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    assert torch.equal(xn2a.view(torch.int16), xn2b.view(torch.int16))
    if mirror:
        assert torch.equal(cata.view(torch.int32), catb.view(torch.int32))
        assert torch.equal(cata[:, C:], xa)
    if next_norm:
        assert torch.equal(xn1a.view(torch.int16), xn1b.view(torch.int16))
