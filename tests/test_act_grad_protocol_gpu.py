"""The protocol of conv2d_gradfix ``_ACT_GRAD_IN_WRITER`` through the modules that set its flags (training/networks.py): a discriminator block
(fromrgb -> conv0 with the skip branch's gradient joined in front of the mask; conv0 -> conv1 with the mask in the filter's transpose) and a
SPADE normalisation (relu(conv_mlp(feat)) -> the gamma | beta convolution), in the per-normalisation form and in the batched form of a SPADE
residual block.  Protocol on against protocol off: the output, the gradient of every input and of every weight must be ``torch.equal``;
bias gradients are summed by a read-only pass and held to rel_err < 1e-4 (tests/test_ops_gpu.py test_bias_act_large); seen on the MI355X: 0 in
every case -- the sum has the unfused path's partial-sum shape (``bias_act._BiasSum`` with ``as_folded``), so it is bit-identical.

The issue's shapes -- one discriminator block at 32 x 32 with 16 channels and batch 2, one ``Spade_Norm_Block`` at 8 x 32 -- run the mask in the
filter's transpose only: their convolutions' input gradients take the fp32 tile, which does not apply it (they fall back to the pass).  The
wider cases (128 channels, batch 9: more than 8192 pixels) run the mask in the convolution's store as well.  How many passes run is counted.

With ``create_graph=True`` (R1's double backward) nothing is fused in the backward pass that records a graph: the consumer applies the
differentiable pass itself, the pass kernels run as often as without the protocol (counted around that call), and first and second
derivatives are identical.  The second backward records nothing, so where it walks the forward graph again the stores may apply the mask."""

import pytest
import torch

from act_grad_cases import count_passes, dgrad_plan, protocol
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _compare(got, want, names):
    worst = 0.0
    for name, u, v in zip(names, got, want):
        assert (u is None) == (v is None), name
        if u is None:
            continue
        if name.endswith('bias'):
            err = rel_err(u, v)
            worst = max(worst, err)
            assert err < 1e-4, (name, err)
        else:
            assert torch.equal(u, v), (name, rel_err(u, v))
    print(f'largest bias-gradient difference {worst:.3g}')


def _run_both(run):
    out = {}
    for on in (False, True):
        with protocol(on), count_passes() as c:
            out[on] = (run(), c.passes)
    return out[False], out[True]


# (channels, batch, passes without the protocol, passes with it): fromrgb, conv0 and conv1 each run one pass without it; with it conv1's
# stays (its output is not deferred), conv0's rides in the filter's transpose, and fromrgb's in conv0's input-gradient launch where a kernel
# applies the mask there (plan kernel 7 without K slices) -- on the fp32 tile conv0 runs the pass for it
@pytest.mark.parametrize('channels,batch,fused_conv', [(16, 2, False), (128, 9, True)], ids=['issue_16ch_batch2', 'wide_128ch_batch9'])
def test_discriminator_block(channels, batch, fused_conv):
    from training import networks
    assert dgrad_plan(batch, channels, channels, 1, 32, 32, 3)[2] == fused_conv
    g = torch.Generator().manual_seed(5)
    net = networks.DiscriminatorBlock(0, channels, channels, resolution=32, img_channels=3, first_layer_idx=0, architecture='resnet', conv_clamp=1.0).cuda()
    with torch.no_grad():
        for p in net.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    img = torch.randn([batch, 3, 32, 32], generator=g).cuda()
    params = list(net.parameters())
    names = ['y', 'img'] + [n for n, _ in net.named_parameters()]

    def first():
        xs = img.clone().requires_grad_(True)
        y = net(None, xs)[0]
        return (y.detach(),) + torch.autograd.grad(y.square().sum(), [xs] + params)

    (want, passes_off), (got, passes_on) = _run_both(first)
    _compare(got, want, names)
    assert passes_off == 3 and passes_on == (1 if fused_conv else 2), (passes_off, passes_on)
    # the clamp of conv0 bites on some elements of these inputs (its mask is what the filter's transpose applies)
    with torch.no_grad():
        h = net.conv0(net.fromrgb(img))
    assert 0 < int((h.abs() >= 1.0).sum()) < h.numel()

    def second():
        xs = img.clone().requires_grad_(True)
        y = net(None, xs)[0]
        with count_passes() as recorded:
            gi = torch.autograd.grad(y.square().sum(), [xs] + params, create_graph=True)
        gg = torch.autograd.grad(gi[0].square().sum(), params, allow_unused=True)
        return (y.detach(),) + tuple(t.detach() for t in gi) + tuple(gg) + (recorded.passes,)

    (want2, passes_off2), (got2, passes_on2) = _run_both(second)
    _compare(got2[:-1], want2[:-1], names + ['dd_' + n for n in names[2:]])
    assert got2[-1] == want2[-1] == 3, (want2[-1], got2[-1])     # the pass kernels run: nothing is fused in a backward pass that records a graph
    assert 3 < passes_on2 <= passes_off2, (passes_off2, passes_on2)


@pytest.mark.parametrize('feat_ch,norm_ch,batch,fused_conv', [(16, 16, 2, False), (32, 64, 36, True)], ids=['issue_8x32', 'wide_batch36'])
def test_spade_norm_block(feat_ch, norm_ch, batch, fused_conv):
    from training import networks
    # the masked launch: the input gradient of the gamma | beta convolution, 2 * norm_ch -> norm_ch hidden channels
    assert dgrad_plan(batch, 2 * norm_ch, norm_ch, 1, 8, 32, 3)[2] == fused_conv
    g = torch.Generator().manual_seed(6)
    net = networks.Spade_Norm_Block(feat_ch, norm_ch).cuda()
    x = torch.randn([batch, norm_ch, 8, 32], generator=g).cuda()
    feat = torch.randn([batch, feat_ch, 8, 32], generator=g).cuda()
    params = list(net.parameters())
    names = ['y', 'x', 'feat'] + [n for n, _ in net.named_parameters()]

    def first():
        xs, fs = x.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        y = net(xs, fs)
        return (y.detach(),) + torch.autograd.grad(y.square().sum(), [xs, fs] + params, allow_unused=True)

    (want, passes_off), (got, passes_on) = _run_both(first)
    _compare(got, want, names)
    assert passes_off == 1 and passes_on == (0 if fused_conv else 1), (passes_off, passes_on)

    def second():
        xs, fs = x.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        y = net(xs, fs)
        with count_passes() as recorded:
            gi = torch.autograd.grad(y.square().sum(), [xs, fs] + params, create_graph=True, allow_unused=True)
        gg = torch.autograd.grad(gi[1].square().sum(), params, allow_unused=True)
        return (y.detach(),) + tuple(None if t is None else t.detach() for t in gi) + tuple(gg) + (recorded.passes,)

    (want2, passes_off2), (got2, passes_on2) = _run_both(second)
    _compare(got2[:-1], want2[:-1], names + ['dd_' + n for n in names[3:]])
    assert got2[-1] == want2[-1] == 1, (want2[-1], got2[-1])
    assert 1 < passes_on2 <= passes_off2, (passes_off2, passes_on2)


def test_spade_resblock_batched_form():
    """``Spade_ResBlockV2._batched_gamma_beta``: the three hidden maps from one convolution, read by one grouped convolution whose input-gradient
    launch (three groups, plan kernel 7 at this size) applies the ReLU's gradient."""
    from training import networks
    batch, ch = 36, 128
    assert dgrad_plan(batch, 3 * 2 * ch, 3 * ch, 3, 8, 32, 3)[2]
    g = torch.Generator().manual_seed(7)
    net = networks.Spade_ResBlockV2(ch, ch, resolution=16, feat_channels=24).cuda()
    x = torch.randn([batch, ch, 8, 32], generator=g).cuda()
    feat = torch.randn([batch, 24, 8, 32], generator=g).cuda()
    params = list(net.parameters())
    names = ['y', 'x', 'feat'] + [n for n, _ in net.named_parameters()]

    def first():
        xs, fs = x.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        y = net(xs * 1.0, fs * 1.0)
        return (y.detach(),) + torch.autograd.grad(y.square().sum(), [xs, fs] + params, allow_unused=True)

    (want, passes_off), (got, passes_on) = _run_both(first)
    _compare(got, want, names)
    assert passes_off - passes_on == 1, (passes_off, passes_on)
