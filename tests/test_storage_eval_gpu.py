"""16-bit activation storage in EVAL mode, and the run-time switch (``training.networks.set_activation_storage``).

Eval mode is what test.py, test_512.py, the snapshot grid and ``recon_full`` run: without a graph every styled layer is the
one-launch modulated convolution (styles in the activation staging, or -- in 16-bit storage for a SINGLE sample only, and for
128 and more output channels -- per-sample weights), demodulation, noise, bias, activation and clamp in its epilogue.
tests/test_storage16_gpu.py holds the TRAINING route to the oracle; here ``GeneratorFull`` and ``GeneratorV18`` (the class inside
released pickles) in bf16 under ``torch.no_grad()`` are held to the oracle run in the same storage type, at batch 1 and at
batch 2 so that both routes are seen.  The oracle takes the route of the block at that batch size (``fused_modconv`` = a single
sample); its V18 restatement does not state the cast of the encoders' inputs, so both sides of that comparison get inputs that
bf16 holds exactly.

Bounds: ``_close`` of tests/test_storage16_gpu.py -- 4e-2 of the largest value and 1.5e-2 rms on every returned tensor, the
project's stated bounds for two bf16 evaluation orders.  The margins measured on one MI355X are in DESIGN 8f.

The switch is held to EXACTNESS: a generator or discriminator switched to a storage type returns ``torch.equal`` outputs to one
constructed with it from the same parameters, in eval and in train mode, and switched back, its own fp32 outputs."""

import pytest
import torch

from oracle import param_fill as PF
from test_storage16_gpu import _close, bf16_oracle, BF16  # noqa: F401  (bf16_oracle is a fixture)

pytestmark = pytest.mark.gpu

KEYS = ('gen_z', 'style_input', 'retain', 'pose', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask', 'denorm_lower_mask')
NAMES = dict(GeneratorFull=('img', 'finetune_img', 'pred_parsing'), GeneratorV18=('img', 'finetune_img', 'upper_mask', 'lower_mask'))


def _kwargs(dtype=None):
    synthesis = dict(PF.G_KWARGS['synthesis_kwargs'], **(dict() if dtype is None else dict(act_dtype=dtype)))
    return dict(PF.G_KWARGS, synthesis_kwargs=synthesis)


def _inputs(kind, n):
    inp = PF.make_inputs(n=n, seed=0)
    if kind == 'GeneratorV18':          # its 60-channel patch stack, as tests/test_models_gpu.py makes it
        inp['style_input'] = PF.make_inputs(n=n, seed=5)['style_input'].repeat(1, 2, 1, 1)[:, :60]
        for k in ('style_input', 'retain', 'pose'):
            inp[k] = inp[k].to(BF16).float()
    return [inp[k] for k in KEYS]


def _margins(what, got, want):
    a, b = got.detach().float().cpu(), want.detach().float().cpu()
    print('%s: largest deviation %.3e of the largest value (bound 4e-2), rms %.3e of the rms (bound 1.5e-2)' % (
        what, float((a - b).abs().max()) / float(b.abs().max()), float((a - b).square().mean().sqrt()) / float(b.square().mean().sqrt())))


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('kind', ['GeneratorFull', 'GeneratorV18'])
def test_eval_mode_in_bf16_storage(bf16_oracle, kind, n):
    from oracle import ref_networks as RN
    from training import networks
    G = PF.fill_module(getattr(networks, kind)(**_kwargs('bfloat16'))).eval().requires_grad_(False)
    assert G.synthesis.act_dtype == BF16 and G.synthesis.b256.use_fp16 and G.synthesis.texture_b256.half_dtype == BF16
    sd = {k: v.detach().clone() for k, v in list(G.named_parameters()) + list(G.named_buffers())}
    args = _inputs(kind, n)
    oracle = RN.generator_full if kind == 'GeneratorFull' else RN.generator_v18
    with torch.no_grad():
        want = oracle(sd, *args, img_resolution=256, conv_clamp=256, mapping_layers=1, noise_mode='const', fused_modconv=(n == 1))
        G = G.cuda()
        got = G(*[a.cuda() for a in args], noise_mode='const')
    assert len(got) == len(want) == len(NAMES[kind])
    for name, a, b in zip(NAMES[kind], got, want):
        assert a.dtype == torch.float32 and a.shape == b.shape and bool(torch.isfinite(a).all()), name
        _margins('%s, batch %d, %s' % (kind, n, name), a, b)
    for name, a, b in zip(NAMES[kind], got, want):
        _close(a, b, (kind, n, name))


def _generator_outputs(G, args, mode):
    G.train(mode == 'train')
    with torch.no_grad():
        return G(*args, noise_mode='const')


@pytest.mark.parametrize('kind', ['GeneratorFull', 'GeneratorV18'])
def test_switched_generator_equals_the_constructed_one(kind):
    from training import networks
    from training.networks import set_activation_storage
    G32 = PF.fill_module(getattr(networks, kind)(**_kwargs())).requires_grad_(False).cuda()
    state = {k: v.clone() for k, v in G32.state_dict().items()}
    outputs = {}
    for n in (1, 2):                    # a single sample takes per-sample weights in eval mode
        args = [a.cuda() for a in _inputs(kind, n)]
        for mode in ('eval', 'train'):
            outputs[n, mode] = _generator_outputs(G32, args, mode)
    for dtype in ('bfloat16', 'float16'):
        built = getattr(networks, kind)(**_kwargs(dtype)).requires_grad_(False).cuda()
        built.load_state_dict(state)
        assert set_activation_storage(G32, dtype) is G32
        for n in (1, 2):
            args = [a.cuda() for a in _inputs(kind, n)]
            for mode in ('eval', 'train'):
                got, want = _generator_outputs(G32, args, mode), _generator_outputs(built, args, mode)
                for name, a, b, c in zip(NAMES[kind], got, want, outputs[n, mode]):
                    assert a.dtype == torch.float32 and bool(torch.isfinite(a).all()), (dtype, n, mode, name)
                    assert torch.equal(a, b), (dtype, n, mode, name, float((a - b).abs().max()))
                    assert not torch.equal(a, c), (dtype, n, mode, name)             # and it is not the fp32 network any more
        del built
    set_activation_storage(G32, None)
    for n in (1, 2):
        args = [a.cuda() for a in _inputs(kind, n)]
        for mode in ('eval', 'train'):
            for name, a, b in zip(NAMES[kind], _generator_outputs(G32, args, mode), outputs[n, mode]):
                assert torch.equal(a, b), ('back to fp32', n, mode, name)
    # (the train-mode calls above moved the mapping network's running mean, as they do in any storage)
    assert all(torch.equal(v, state[k]) for k, v in G32.state_dict().items() if k != 'mapping.w_avg')


def test_switched_discriminator_equals_the_constructed_one():
    from training import networks
    from training.networks import set_activation_storage
    D32 = PF.fill_module(networks.Discriminator(**PF.D_KWARGS)).requires_grad_(False).cuda()
    state = {k: v.clone() for k, v in D32.state_dict().items()}
    inp = PF.make_inputs(n=4, seed=1)
    c = torch.tanh(inp['style_input'].mean(dim=[2, 3]).repeat(1, 13)[:, :512]).cuda()
    x = inp['real_img'].cuda()
    with torch.no_grad():
        logits32 = D32(x, c)
    for dtype in ('bfloat16', 'float16'):
        built = networks.Discriminator(**PF.D_KWARGS, half_dtype=dtype, num_fp16_res=6).requires_grad_(False).cuda()
        built.load_state_dict(state)
        set_activation_storage(D32, dtype)
        with torch.no_grad():
            got, want = D32(x, c), built(x, c)
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), (dtype, float((got - want).abs().max()))
        assert not torch.equal(got, logits32), dtype
    set_activation_storage(D32, 'float32')
    with torch.no_grad():
        assert torch.equal(D32(x, c), logits32)
    assert all(torch.equal(v, state[k]) for k, v in D32.state_dict().items())
