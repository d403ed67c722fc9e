"""The data-parallel training step of PASTA-GAN's full-body model.

Mirrors the hot loop of the reference's training/training_loop_wo_flow_fullbody.py: module
construction (:274-277), replica synchronisation and gradient exchange (:312-324), lazily regularised Adam
phases Gmain/Greg/Dmain/Dreg (:332-349), gradient accumulation with ``sync`` only on the last round
(:484-505), gradient ``nan_to_num`` + optimiser step (:508-516) and the generator EMA (:521-529).
One process per GPU; gradients are all-reduced by RCCL (``backend='nccl'`` on ROCm) over xGMI, overlapped
with backward: by default through one ``FlatGradReducer`` per optimised module (``ddp_mode='flat'``,
training/grad_reducer.py), or through the reference's five DistributedDataParallel wrappers (``ddp_mode='torch'``).

With a ``run_dir``, ``training_loop`` is the reference's whole loop (:247-654): ticks counted in kimg, the status line,
stats.jsonl, the sample-image grid (training/snapshot_grid.py), network snapshots, resuming and aborting, and -- beyond the
reference -- a training-state file per network snapshot from which a run continues bit for bit (training/train_state.py); the statistics
accumulate on the device (torch_utils/training_stats.py) and none of it touches ``TrainingStep.run``'s arithmetic.  With
``metrics``, every network snapshot is scored on all ranks (metrics/; the reference has this call commented out, :604-614).
``SyntheticFullBodyBatch`` supplies tensors of the dataset's shapes (training_loop...:289-297, 425-456)
directly in HBM; with ``training_set_kwargs``, ``training_loop`` reads the reference's data set
(training/dataset.py) and prepares each batch on the GPU (training/tryon_batch.py).
"""

import copy
import json
import os
import pickle
import time

import numpy as np
import torch

import dnnlib
from torch_utils import misc
from torch_utils import training_stats
from training.grad_reducer import FlatGradReducer, broadcast_module_states

#----------------------------------------------------------------------------

AUGPIPE_SPECS = {    # train_wo_flow_fullbody.py:297-309: which AugmentPipe multipliers each --augpipe name switches on
    'blit':   ['xflip', 'rotate90', 'xint'],
    'geom':   ['scale', 'rotate', 'aniso', 'xfrac'],
    'color':  ['brightness', 'contrast', 'lumaflip', 'hue', 'saturation'],
    'filter': ['imgfilter'],
    'noise':  ['noise'],
    'cutout': ['cutout'],
}
for _name, _parts in [('bg', ['blit', 'geom']), ('bgc', ['blit', 'geom', 'color']), ('bgcf', ['blit', 'geom', 'color', 'filter']),
                      ('bgcfn', ['blit', 'geom', 'color', 'filter', 'noise']), ('bgcfnc', ['blit', 'geom', 'color', 'filter', 'noise', 'cutout'])]:
    AUGPIPE_SPECS[_name] = [m for part in _parts for m in AUGPIPE_SPECS[part]]

def augment_options(aug='ada', augpipe='bgc', p=None, target=None):
    """The --aug / --p / --target / --augpipe options (train_wo_flow_fullbody.py:249-313) as TrainingStep config entries:
    'ada' adapts p towards ``target`` (default 0.6) from ``p`` (default 0); 'fixed' keeps ``p``; 'noaug' -> {}."""
    if aug == 'noaug':
        return dnnlib.EasyDict()
    assert aug in ('ada', 'fixed') and augpipe in AUGPIPE_SPECS
    assert aug != 'fixed' or p is not None, '--aug=fixed requires p'
    opts = dnnlib.EasyDict(augment_kwargs=dnnlib.EasyDict(class_name='training.augment.AugmentPipe', **{m: 1 for m in AUGPIPE_SPECS[augpipe]}),
                           augment_p=float(p) if p is not None else 0.0)
    if aug == 'ada':
        opts.ada_target = 0.6 if target is None else float(target)
    return opts

def fashion_config(channel_base=16384, d_fp16_res=0, mbstd_group_size=4, img_resolution=256, act_dtype=None):
    """G/D/optimiser/loss options of ``--cfg fashion`` (train_wo_flow_fullbody.py:166-215, train.sh:3-10); augmentation
    off (``cfg.update(augment_options(...))`` turns it on).  ``act_dtype`` ('bfloat16' / 'float16'; BASELINE config 5):
    16-bit activation storage in the generator's synthesis network and encoders and in every discriminator block."""
    G_kwargs = dnnlib.EasyDict(class_name='training.networks.GeneratorFull', z_dim=0, c_dim=512, w_dim=512, img_resolution=img_resolution,
                               img_channels=3, mapping_kwargs=dnnlib.EasyDict(num_layers=1),
                               synthesis_kwargs=dnnlib.EasyDict(channel_base=channel_base, channel_max=512, num_fp16_res=3,
                                                                conv_clamp=256, use_noise=True))
    D_kwargs = dnnlib.EasyDict(class_name='training.networks.Discriminator', c_dim=512, img_resolution=img_resolution, img_channels=3,
                               channel_base=channel_base, channel_max=512, num_fp16_res=d_fp16_res, conv_clamp=256,
                               block_kwargs=dnnlib.EasyDict(), mapping_kwargs=dnnlib.EasyDict(),
                               epilogue_kwargs=dnnlib.EasyDict(mbstd_group_size=mbstd_group_size))
    if act_dtype is not None:
        G_kwargs.synthesis_kwargs.act_dtype = act_dtype
        D_kwargs.half_dtype = act_dtype
        D_kwargs.num_fp16_res = int(np.log2(img_resolution)) - 2      # every block b<R> .. b8
    opt = dnnlib.EasyDict(class_name='torch.optim.Adam', lr=0.002, betas=[0, 0.99], eps=1e-8)
    loss_kwargs = dnnlib.EasyDict(class_name='training.loss_wo_flow_fullbody.StyleGAN2Loss', r1_gamma=10, l1_weight=40,
                                  vgg_weight=0, contextual_weight=0, pl_weight=0, mask_weight=20)
    return dnnlib.EasyDict(G_kwargs=G_kwargs, D_kwargs=D_kwargs, G_opt_kwargs=opt, D_opt_kwargs=dnnlib.EasyDict(opt),
                           loss_kwargs=loss_kwargs, ema_kimg=10, ema_rampup=None, G_reg_interval=4, D_reg_interval=16)

#----------------------------------------------------------------------------

class SyntheticFullBodyBatch:
    """Device-resident synthetic batch with the dataset's tensor shapes and value ranges."""
    KEYS = ['real_img', 'style_input', 'retain', 'pose', 'denorm_upper_input', 'denorm_lower_input',
            'denorm_upper_mask', 'denorm_lower_mask', 'gt_parsing']

    def __init__(self, batch, device, seed=0, res=256):
        g = torch.Generator(device='cpu').manual_seed(1234 + seed)
        n = batch
        def u(*shape):
            return torch.rand(shape, generator=g) * 2 - 1
        def blobs(p):
            coarse = torch.rand([n, 1, res // 16, res // 16], generator=g)
            return (torch.nn.functional.interpolate(coarse, size=(res, res), mode='bilinear', align_corners=False) < p).float()
        real_img = u(n, 3, res, res)
        real_img[..., : res // 8] = 1.0               # 192-wide content, white padded to a square (dataset.py:520-524)
        real_img[..., res - res // 8:] = 1.0
        mask = blobs(0.5)
        retain = mask * real_img - (1 - mask)
        lines = (torch.rand([n, 3, res, res], generator=g) < 0.02).float() * 2 - 1
        style = u(n, 42, res // 4, res // 4)
        drop = (torch.rand([n, 14, 1, 1], generator=g) < 0.3).repeat_interleave(3, dim=1)
        style = torch.where(drop, -torch.ones_like(style), style)
        du_mask, dl_mask = blobs(0.35), blobs(0.35)
        gt = torch.randint(0, 6, [n, 1, res // 8, res // 8], generator=g).float()
        t = dict(real_img=real_img, style_input=style, retain=retain, pose=torch.cat([lines, retain], dim=1),
                 denorm_upper_input=u(n, 3, res, res) * du_mask - (1 - du_mask),
                 denorm_lower_input=u(n, 3, res, res) * dl_mask - (1 - dl_mask),
                 denorm_upper_mask=du_mask, denorm_lower_mask=dl_mask,
                 gt_parsing=torch.nn.functional.interpolate(gt, size=(res, res), mode='nearest'))
        self.tensors = {k: v.to(device) for k, v in t.items()}
        self.batch = n

    def split(self, batch_gpu):
        parts = {k: v.split(batch_gpu) for k, v in self.tensors.items()}
        return [{k: parts[k][i] for k in self.KEYS} for i in range(len(parts['real_img']))]

#----------------------------------------------------------------------------

class TrainingStep:
    """Owns G, D, G_ema, the DDP wrappers, the loss and the four optimiser phases; ``run()`` executes one
    iteration of the reference's hot loop on a device-resident batch."""

    def __init__(self, device, cfg=None, num_gpus=1, rank=0, batch_size=16, batch_gpu=16, random_seed=0, ddp_bucket_mb=None, ddp_mode='flat',
                 resume_data=None):
        cfg = cfg if cfg is not None else fashion_config(mbstd_group_size=min(batch_gpu, 4))
        assert ddp_mode in ('flat', 'torch')
        self.device, self.num_gpus, self.rank = device, num_gpus, rank
        self.batch_size, self.batch_gpu = batch_size, batch_gpu
        assert batch_size % (batch_gpu * num_gpus) == 0
        np.random.seed(random_seed * num_gpus + rank)
        torch.manual_seed(random_seed * num_gpus + rank)
        # allow_tf32 (training_loop_wo_flow_fullbody.py:243, 253-254; default False): the reference lets cuDNN / cuBLAS round
        # operands to TF32.  gfx950 has no TF32 matrix instructions; the counterpart here is the three-product split-bf16
        # arithmetic (2^-16 relative, against TF32's 2^-11) at half of the default mode's matrix work.
        if cfg.get('allow_tf32', False):
            from torch_utils.ops import conv2d_gradfix
            conv2d_gradfix.conv_math = 'bf16x3'

        self.G = dnnlib.util.construct_class_by_name(**cfg.G_kwargs).train().requires_grad_(False).to(device)
        self.D = dnnlib.util.construct_class_by_name(**cfg.D_kwargs).train().requires_grad_(False).to(device)
        self.G_ema = copy.deepcopy(self.G).eval()
        self.ema_kimg, self.ema_rampup = cfg.ema_kimg, cfg.ema_rampup
        if resume_data is not None and rank == 0:      # :280-285, before the replicas take rank 0's state below
            for name, module in [('G', self.G), ('D', self.D), ('G_ema', self.G_ema)]:
                misc.copy_params_and_buffers(resume_data[name], module, require_all=False)

        # Replicas: rank 0's state everywhere, then a gradient exchange per optimised module.
        #   'flat'  - one FlatGradReducer for G and one for D (64 MiB buckets: G = 3 all-reduces, D = 2), gated by this
        #             class on the last accumulation round; the loss sees plain modules, its ddp_sync calls are no-ops.
        #   'torch' - the reference's arrangement (:316-324): one DistributedDataParallel wrapper per sub-module so that
        #             the loss can gate their all-reduces separately with ddp_sync; find_unused_parameters only where a
        #             parameter really takes no gradient (G.synthesis: b4.const; the parsing head when mask_weight = 0).
        G, D = self.G, self.D
        ddp = dict(G_mapping=G.mapping, G_synthesis=G.synthesis, G_const_encoding=G.const_encoding,
                   G_style_encoding=G.style_encoding, D=D)
        self.reducers = {}
        if num_gpus > 1 and ddp_mode == 'flat':
            with torch.no_grad():
                broadcast_module_states([G, D, self.G_ema])
            for name, module in [('G', G), ('D', D)]:
                if any(True for _ in module.parameters()):
                    self.reducers[name] = FlatGradReducer(module, num_gpus, bucket_mb=ddp_bucket_mb or 64)
        elif num_gpus > 1:
            for name, module in list(ddp.items()) + [(None, self.G_ema)]:
                if len(list(module.parameters())) != 0:
                    module.requires_grad_(True)
                    ids = [device] if device.type == 'cuda' else None
                    module = torch.nn.parallel.DistributedDataParallel(module, device_ids=ids, broadcast_buffers=False,
                                                                       find_unused_parameters=(name == 'G_synthesis'),
                                                                       bucket_cap_mb=ddp_bucket_mb or 25)
                    module.requires_grad_(False)
                if name is not None:
                    ddp[name] = module
        self.ddp_modules = ddp

        # ADA (training_loop_wo_flow_fullbody.py:301-310): the pipeline, its probability p, and the statistic that steers p
        self.augment_pipe = None
        self.ada_target, self.ada_interval, self.ada_kimg = cfg.get('ada_target'), cfg.get('ada_interval', 4), cfg.get('ada_kimg', 500)
        loss_kwargs = dict(cfg.loss_kwargs)
        if cfg.get('augment_kwargs') is not None and (cfg.get('augment_p', 0) > 0 or self.ada_target is not None):
            self.augment_pipe = dnnlib.util.construct_class_by_name(**cfg.augment_kwargs).train().requires_grad_(False).to(device)
            self.augment_pipe.p.copy_(torch.as_tensor(float(cfg.get('augment_p', 0))))
            if self.ada_target is not None:
                # sum and count of sign(D(real)) since the last adjustment, kept on the device (the reference's
                # training_stats.Collector(regex='Loss/signs/real') reads them back to the host every ada_interval)
                self._ada_acc = torch.zeros([2], device=device)
                user_report = loss_kwargs.get('report_fn')
                def report(name, value):
                    if name == 'Loss/signs/real':
                        v = value.detach().float()
                        self._ada_acc += torch.stack([v.sum(), torch.full([], float(v.numel()), device=v.device)])
                    if user_report is not None:
                        user_report(name, value)
                loss_kwargs['report_fn'] = report
        self.loss = dnnlib.util.construct_class_by_name(device=device, **ddp, augment_pipe=self.augment_pipe, **loss_kwargs)

        self.phases = []
        for name, module, opt_kwargs, reg_interval in [('G', G, cfg.G_opt_kwargs, cfg.G_reg_interval), ('D', D, cfg.D_opt_kwargs, cfg.D_reg_interval)]:
            if (device.type == 'cuda' and opt_kwargs.get('class_name') == 'torch.optim.Adam' and 'fused' not in opt_kwargs
                    and 'foreach' not in opt_kwargs):
                # the same update (torch.optim.Adam's formula) as ONE multi-tensor kernel per step instead of seven foreach passes
                opt_kwargs = dnnlib.EasyDict(opt_kwargs, fused=True)
            if reg_interval is None:
                opt = dnnlib.util.construct_class_by_name(params=module.parameters(), **opt_kwargs)
                self.phases += [dnnlib.EasyDict(name=name + 'both', module=module, opt=opt, interval=1)]
            else:   # lazy regularisation (:337-346)
                mb_ratio = reg_interval / (reg_interval + 1)
                opt_kwargs = dnnlib.EasyDict(opt_kwargs)
                opt_kwargs.lr = opt_kwargs.lr * mb_ratio
                opt_kwargs.betas = [beta ** mb_ratio for beta in opt_kwargs.betas]
                opt = dnnlib.util.construct_class_by_name(module.parameters(), **opt_kwargs)
                self.phases += [dnnlib.EasyDict(name=name + 'main', module=module, opt=opt, interval=1)]
                self.phases += [dnnlib.EasyDict(name=name + 'reg', module=module, opt=opt, interval=reg_interval)]
        for phase in self.phases:           # set by whoever wants phase timings (:344-349); recorded in run() when present
            phase.start_event = phase.end_event = None
            phase.timed = False             # the events have been recorded (a continued run has not yet run every phase at its first tick)
        self.batch_idx = 0
        self.cur_nimg = 0
        self._buf_versions = {}         # G buffer index -> version counter at its last copy into G_ema

    def run(self, data):
        """One iteration: every due phase accumulates gradients over the local rounds, then steps its optimiser;
        finally the EMA generator is updated. ``data`` is a ``SyntheticFullBodyBatch`` holding this rank's
        ``batch_size // num_gpus`` samples."""
        rounds = data.split(self.batch_gpu)
        z_dim = self.G.z_dim
        all_gen_z = torch.randn([len(self.phases), len(rounds) * self.batch_gpu, z_dim], device=self.device)
        for phase, phase_gen_z in zip(self.phases, all_gen_z):
            if self.batch_idx % phase.interval != 0:
                continue
            reducer = self.reducers.get(phase.name[0])
            if phase.start_event is not None:
                phase.start_event.record(torch.cuda.current_stream(self.device))
            phase.module.requires_grad_(True)
            if reducer is not None:
                reducer.begin()
            else:
                phase.opt.zero_grad(set_to_none=True)
            for round_idx, (r, gen_z) in enumerate(zip(rounds, phase_gen_z.split(self.batch_gpu))):
                sync = (round_idx == self.batch_size // (self.batch_gpu * self.num_gpus) - 1)
                if reducer is not None and sync:     # the exchange overlaps the backward pass(es) of the last round
                    reducer.arm(getattr(self.loss, 'backward_passes', lambda phase: None)(phase.name))
                self.loss.accumulate_gradients(phase=phase.name, gen_z=gen_z, sync=sync, gain=phase.interval, **r)
            phase.module.requires_grad_(False)
            if reducer is not None:
                reducer.finish()
                grads = reducer.flat_gradients()
            else:
                grads = [param.grad for param in phase.module.parameters() if param.grad is not None]
            if grads:       # nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5) (:513-515), one launch per 96 gradients
                misc.nan_to_num_(grads, nan=0, posinf=1e5, neginf=-1e5)
            phase.opt.step()
            if phase.end_event is not None:
                phase.end_event.record(torch.cuda.current_stream(self.device))
                phase.timed = True

        ema_nimg = self.ema_kimg * 1000
        if self.ema_rampup is not None:
            ema_nimg = min(ema_nimg, self.cur_nimg * self.ema_rampup)
        ema_beta = 0.5 ** (self.batch_size / max(ema_nimg, 1e-8))
        with torch.no_grad():
            # p_ema <- p.lerp(p_ema, beta) (:522-529), as one multi-tensor launch: p_ema + (1 - beta) * (p - p_ema)
            torch._foreach_lerp_(list(self.G_ema.parameters()), list(self.G.parameters()), 1.0 - ema_beta)
            # b_ema.copy_(b) for every buffer (:528-529).  Only w_avg ever changes; a buffer whose version counter has not
            # moved since its last copy still equals its copy, so it is skipped (~75 tiny device copies per iteration).
            src, dst = [], []
            for i, (b_ema, b) in enumerate(zip(self.G_ema.buffers(), self.G.buffers())):
                if self._buf_versions.get(i) != b._version:
                    src.append(b); dst.append(b_ema)
                    self._buf_versions[i] = b._version
            if src:
                torch._foreach_copy_(dst, src)
        self.cur_nimg += self.batch_size

        # ADA adjustment (:536-539): p += sign(E[sign(D(real))] - target) * batch_size * ada_interval / (ada_kimg * 1000), p >= 0;
        # evaluated on the device, no read-back
        self.batch_idx += 1
        if self.augment_pipe is not None and self.ada_target is not None and self.batch_idx % self.ada_interval == 0:
            acc = self._ada_acc
            if self.num_gpus > 1:
                torch.distributed.all_reduce(acc)
            step = (self.batch_size * self.ada_interval) / (self.ada_kimg * 1000)
            mean = acc[0] / acc[1].clamp(min=1)
            adjust = torch.sign(mean - self.ada_target) * step * (acc[1] > 0)
            self.augment_pipe.p.copy_((self.augment_pipe.p + adjust).clamp(min=0))
            acc.zero_()

#----------------------------------------------------------------------------

def _numbered_batches(loader, people_jitter, random_seed, num_gpus, rank, cur_nimg, erase_strokes=None):
    """The collated batches of ``loader`` numbered: the int64 positions [N] its items have in the sampler's global stream, with the
    run's seed, attached as ``raw['jitter']`` with the specification ``people_jitter`` (``--jitter-people``) and, through
    ``attach_strokes``, as ``raw['erase_strokes']`` with the specification ``erase_strokes`` (``--erase-masks strokes``); either
    may be None.  Position ``t`` belongs to rank ``t % num_gpus`` and a rank reads its positions in increasing order from
    ``cur_nimg`` (``InfiniteSampler(skip=)``), so a continued run numbers its items as the uninterrupted one does."""
    from training.tryon_batch import attach_strokes
    t = cur_nimg + (rank - cur_nimg) % num_gpus             # the rank's first position at or after cur_nimg
    for raw in loader:
        n = int(raw['raw_idx'].shape[0])
        positions = t + num_gpus * np.arange(n, dtype=np.int64)
        if people_jitter is not None:
            raw['jitter'] = dict(spec=dict(people_jitter), seed=int(random_seed), positions=positions)
        if erase_strokes is not None:
            attach_strokes(raw, erase_strokes, random_seed, positions)
        t += num_gpus * n
        yield raw

def _data_batches(num_gpus, rank, batch_size, random_seed, device, training_set_kwargs, data_loader_kwargs, cur_nimg=0, people_jitter=None,
                  swap_outfits=None, part_geometry='host'):
    """(training_set, builder, iterator over prepared batches) of the reference's data set (:261-263).  ``cur_nimg``: the images
    a continued run has consumed; one iteration takes ``batch_size`` positions of the sampler's global stream whatever the
    number of ranks, so the stream goes on at that position.  ``people_jitter``: a specification of
    ``training.tryon_batch.jitter_spec``; the batches are then numbered (``_numbered_batches``) and the builder jitters them.  A
    data set opened with ``erase_masks='strokes'`` has its batches numbered as well, with or without the jitter, and the builder
    draws their erase masks.  ``swap_outfits``: dict(region=, group=) of training/swap_outfits.py; every batch then also carries the
    swapped inputs of the unpaired pass, made from its own stages after the mirroring and the jitter.  ``part_geometry``: 'host' or
    'gpu' (``--part-geometry``), where the batches' body-part matrices are solved; the builder RETURNED is always the
    host's, since it serves the sample grid, which keeps the host geometry."""
    from training import dataset as dataset_module
    from training.tryon_batch import builder_for, jitter_spec
    training_set = dnnlib.util.construct_class_by_name(**training_set_kwargs)
    sampler = misc.InfiniteSampler(dataset=training_set, rank=rank, num_replicas=num_gpus, seed=random_seed, skip=cur_nimg)
    loader = torch.utils.data.DataLoader(dataset=training_set, sampler=sampler, batch_size=batch_size // num_gpus,
                                         collate_fn=dataset_module.collate, **(data_loader_kwargs or {}))
    grid_builder = builder_for(training_set, device)
    builder = builder_for(training_set, device, part_geometry) if part_geometry != 'host' else grid_builder
    erase_strokes = training_set.erase_strokes if getattr(training_set, 'erase_masks', 'files') == 'strokes' else None
    if people_jitter is not None or erase_strokes is not None:
        loader = _numbered_batches(loader, jitter_spec(people_jitter) if people_jitter is not None else None, random_seed, num_gpus, rank,
                                   int(cur_nimg), erase_strokes=erase_strokes)
    if swap_outfits is not None:
        swap_outfits = dict(swap_outfits)
        return training_set, grid_builder, (builder.build(raw, swap=swap_outfits) for raw in loader)
    return training_set, grid_builder, (builder.build(raw) for raw in loader)

def training_loop(num_gpus=1, rank=0, batch_size=16, batch_gpu=16, random_seed=0, total_iters=4, cfg=None, device=None, progress_fn=None,
                  training_set_kwargs=None, data_loader_kwargs=None, run_dir=None, total_kimg=25000, kimg_per_tick=4,
                  image_snapshot_ticks=50, network_snapshot_ticks=50, resume_pkl=None, abort_fn=None, snapshot_gnum=23, metrics=None,
                  metric_set_kwargs=None, save_state=False, resume_state=None, people_jitter=None, swap_outfits=None, part_geometry='host'):
    """Without ``run_dir``: run ``total_iters`` iterations and write nothing.  Without ``training_set_kwargs`` the data is
    synthetic; with them the data set is built by ``construct_class_by_name`` (e.g. ``class_name='training.dataset.UvitonDatasetFull',
    path=...``) and read through an InfiniteSampler and a DataLoader (:147-152), each batch prepared on the GPU by
    ``training.tryon_batch.builder_for``'s builder (``UvitonDatasetFull_512``: the 512 x 320 one).
    With ``run_dir`` (and a data set): the reference's loop until ``total_kimg`` (``training_run`` below); ``total_iters`` is unused.
    ``metrics`` (names of metrics/metric_main.py) are evaluated on G_ema after every network snapshot, on ``metric_set_kwargs``
    (default: the training set's).
    ``save_state``: every tick that writes a network snapshot also writes ``training-state-<kimg>.pt`` (training/train_state.py),
    the newest one kept.  ``resume_state``: the path of such a file; the run goes on from it exactly where the other stopped.
    The state file records the text of ``run_dir``'s training_options.json, when the command line has written one, for ``--continue``.
    ``people_jitter``: a specification of ``training.tryon_batch.jitter_spec`` (``--jitter-people``); the training batches, and only
    they, are jittered per item by the run's seed and the item's position in the sampler's stream.
    ``swap_outfits``: dict(region=, group=) (``--swap_weight``, ``--swap-region``); the training batches, and only they,
    also carry every person in a batch-mate's garments, which a loss with ``swap_weight > 0`` trains on.
    ``part_geometry``: 'host' or 'gpu' (``--part-geometry``): where the training batches' body-part matrices are solved;
    the sample grid and the metrics keep the host's."""
    device = device if device is not None else torch.device('cuda', rank)
    if resume_state is not None and run_dir is None:
        raise ValueError('resume_state needs a run_dir: only a training run is continued')
    if resume_state is not None and resume_pkl is not None:
        raise ValueError(f'resume_state={resume_state!r} and resume_pkl={resume_pkl!r}: a continued run takes its networks from the state file')
    if run_dir is not None:
        return training_run(run_dir, num_gpus, rank, batch_size, batch_gpu, random_seed, cfg, device, progress_fn, training_set_kwargs,
                            data_loader_kwargs, total_kimg, kimg_per_tick, image_snapshot_ticks, network_snapshot_ticks, resume_pkl, abort_fn,
                            snapshot_gnum, metrics, metric_set_kwargs, save_state, resume_state, people_jitter, swap_outfits, part_geometry)
    step = TrainingStep(device, cfg=cfg, num_gpus=num_gpus, rank=rank, batch_size=batch_size, batch_gpu=batch_gpu, random_seed=random_seed)
    if training_set_kwargs is None:
        data = SyntheticFullBodyBatch(batch_size // num_gpus, device, seed=rank)
        batches = iter(lambda: data, None)
    else:
        _, _, batches = _data_batches(num_gpus, rank, batch_size, random_seed, device, training_set_kwargs, data_loader_kwargs,
                                      people_jitter=people_jitter, swap_outfits=swap_outfits, part_geometry=part_geometry)
    for it in range(total_iters):
        step.run(next(batches))
        if progress_fn is not None:
            progress_fn(it + 1, total_iters)
    return step

#----------------------------------------------------------------------------

def sample_images(G_ema, grid, grid_z, batch_gpu):
    """G_ema's try-on images over the grid (:580-583), one ``batch_gpu`` minibatch at a time: a generator of fp32 [n, 3, H, H]."""
    with torch.no_grad():
        for i, z in enumerate(grid_z):
            lo = i * batch_gpu
            yield G_ema(z=z, **grid.inputs(lo, lo + int(z.shape[0])), noise_mode='const')[1]

def training_run(run_dir, num_gpus, rank, batch_size, batch_gpu, random_seed, cfg, device, progress_fn, training_set_kwargs, data_loader_kwargs,
                 total_kimg, kimg_per_tick, image_snapshot_ticks, network_snapshot_ticks, resume_pkl, abort_fn, snapshot_gnum, metrics=None,
                 metric_set_kwargs=None, save_state=False, resume_state=None, people_jitter=None, swap_outfits=None, part_geometry='host'):
    """The reference's training_loop (:247-654) around ``TrainingStep.run``.  Returns the step; on rank 0 it carries the
    ``snapshot_grid`` and the ``grid_z`` the sample images were drawn with."""
    import psutil
    from training import train_state
    start_time = launch_time = time.time()
    state = None
    if resume_state is not None:        # every rank reads the file: its own generators and w_avg are in it
        state = train_state.load_state(resume_state)
        train_state.check_run(state, num_gpus=num_gpus, batch_size=batch_size, batch_gpu=batch_gpu, random_seed=random_seed)
        start_time -= float(state['elapsed_sec'])       # Timing/total_* go on from the wall clock of the run so far
    options_json = ''
    if save_state and rank == 0 and os.path.isfile(os.path.join(run_dir, 'training_options.json')):
        with open(os.path.join(run_dir, 'training_options.json'), 'rt') as f:
            options_json = f.read()
    if training_set_kwargs is None:
        raise ValueError('a training run needs training_set_kwargs: the sample grid is made of the data set\'s train_img_vis people')
    cfg = dnnlib.EasyDict(cfg if cfg is not None else fashion_config(mbstd_group_size=min(batch_gpu, 4)))
    cfg.loss_kwargs = dnnlib.EasyDict(cfg.loss_kwargs, report_fn=training_stats.report)

    if rank == 0:
        print('Loading training set...')
    training_set, builder, batches = _data_batches(num_gpus, rank, batch_size, random_seed, device, training_set_kwargs, data_loader_kwargs,
                                                   cur_nimg=int(state['cur_nimg']) if state is not None else 0, people_jitter=people_jitter,
                                                   swap_outfits=swap_outfits, part_geometry=part_geometry)
    if rank == 0:
        print()
        print('Num images: ', len(training_set))
        print('Image shape:', training_set.image_shape)
        print()

    resume_data = None
    if resume_pkl is not None and rank == 0:
        import legacy
        print(f'Resuming from "{resume_pkl}"')
        with open(resume_pkl, 'rb') as f:
            resume_data = legacy.load_network_pkl(f)
    if rank == 0:
        print('Constructing networks...')
    step = TrainingStep(device, cfg=cfg, num_gpus=num_gpus, rank=rank, batch_size=batch_size, batch_gpu=batch_gpu, random_seed=random_seed,
                        resume_data=resume_data)
    del resume_data
    G, D, G_ema, augment_pipe = step.G, step.D, step.G_ema, step.augment_pipe
    if rank == 0:
        for phase in step.phases:
            phase.start_event = torch.cuda.Event(enable_timing=True)
            phase.end_event = torch.cuda.Event(enable_timing=True)

    grid = None
    if rank == 0:
        from training.snapshot_grid import SnapshotGrid
        print('Exporting sample images...')
        grid = SnapshotGrid.setup(training_set, builder, device, gnum=snapshot_gnum)
        grid.save_init(run_dir)
        step.snapshot_grid = grid
        if state is None:
            step.grid_z = torch.randn([grid.cells, G.z_dim], device=device).split(batch_gpu)       # drawn once (:376)
        else:
            if tuple(state['grid_z'].shape) != (grid.cells, G.z_dim):
                raise ValueError(f'grid_z: {tuple(state["grid_z"].shape)} in the state file, this run\'s grid needs {(grid.cells, G.z_dim)}')
            step.grid_z = state['grid_z'].to(device).split(batch_gpu)
    if state is not None:
        if rank == 0:
            print(f'Continuing from "{resume_state}"')
        train_state.restore(step, state)

    if rank == 0:
        print('Initializing logs...')
    stats_collector = training_stats.Collector(regex='.*')
    stats_metrics = dict()
    stats_jsonl = None
    stats_tfevents = None
    if rank == 0:
        stats_jsonl = open(os.path.join(run_dir, 'stats.jsonl'), 'w')
        try:
            import torch.utils.tensorboard as tensorboard
            stats_tfevents = tensorboard.SummaryWriter(run_dir)
        except ImportError as err:
            print('Skipping tfevents export:', err)

    if rank == 0:
        print(f'Training for {total_kimg} kimg...')
        print()
    total_nimg = total_kimg * 1000
    cur_tick = int(state['cur_tick']) if state is not None else 0
    tick_start_nimg = step.cur_nimg
    tick_start_time = time.time()
    maintenance_time = tick_start_time - launch_time
    if progress_fn is not None:
        progress_fn(0, total_kimg)
    while True:
        if step.cur_nimg < total_nimg:          # total_kimg = 0: no iteration at all, one tick of maintenance (a resumed state written back)
            batch = next(batches)
            if state is not None:               # the generators last of all: the first fetch starts the loader, which draws its base seed
                train_state.restore_rng(step, state)
                state = None
            step.run(batch)
        elif state is not None:                 # nothing left to train: the state written below carries the generators on
            train_state.restore_rng(step, state)
            state = None
        cur_nimg = step.cur_nimg

        # Perform maintenance tasks once per tick.
        done = (cur_nimg >= total_nimg)
        if (not done) and (cur_tick != 0 or resume_state is not None) and (cur_nimg < tick_start_nimg + kimg_per_tick * 1000):
            continue        # (a continued run has no tick 0: its first maintenance round is the next regular tick)

        # Print status line, accumulating the same information in stats_collector.
        tick_end_time = time.time()
        report0 = training_stats.report0
        fields = []
        fields += [f"tick {report0('Progress/tick', cur_tick):<5d}"]
        fields += [f"kimg {report0('Progress/kimg', cur_nimg / 1e3):<8.1f}"]
        fields += [f"time {dnnlib.util.format_time(report0('Timing/total_sec', tick_end_time - start_time)):<12s}"]
        fields += [f"sec/tick {report0('Timing/sec_per_tick', tick_end_time - tick_start_time):<7.1f}"]
        fields += [f"sec/kimg {report0('Timing/sec_per_kimg', (tick_end_time - tick_start_time) / max(cur_nimg - tick_start_nimg, 1) * 1e3):<7.2f}"]
        fields += [f"maintenance {report0('Timing/maintenance_sec', maintenance_time):<6.1f}"]
        fields += [f"cpumem {report0('Resources/cpu_mem_gb', psutil.Process(os.getpid()).memory_info().rss / 2**30):<6.2f}"]
        fields += [f"gpumem {report0('Resources/peak_gpu_mem_gb', torch.cuda.max_memory_allocated(device) / 2**30):<6.2f}"]
        torch.cuda.reset_peak_memory_stats(device)
        fields += [f"augment {report0('Progress/augment', float(augment_pipe.p.cpu()) if augment_pipe is not None else 0):.3f}"]
        report0('Timing/total_hours', (tick_end_time - start_time) / (60 * 60))
        report0('Timing/total_days', (tick_end_time - start_time) / (24 * 60 * 60))
        if rank == 0:
            print(' '.join(fields))

        # Check for abort.
        abort = (not done) and (abort_fn is not None) and bool(abort_fn())
        if num_gpus > 1 and abort_fn is not None:       # one answer for all ranks: a rank that stopped alone would leave the others waiting
            flag = torch.tensor([int(abort)], dtype=torch.int32, device=device)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
            abort = (not done) and bool(flag.item())
        if abort:
            done = True
            if rank == 0:
                print()
                print('Aborting...')

        # Save image snapshot.
        if (rank == 0) and (image_snapshot_ticks is not None) and (done or cur_tick % image_snapshot_ticks == 0):
            grid.save(sample_images(G_ema, grid, step.grid_z, batch_gpu), os.path.join(run_dir, f'fakes{cur_nimg//1000:06d}_finetune.png'))

        # Save network snapshot.
        snapshot_pkl = None
        if (network_snapshot_ticks is not None) and (done or cur_tick % network_snapshot_ticks == 0):
            snapshot_data = dict(training_set_kwargs=dict(training_set_kwargs))
            for name, module in [('G', G), ('D', D), ('G_ema', G_ema), ('augment_pipe', augment_pipe)]:
                if module is not None:
                    if num_gpus > 1:
                        misc.check_ddp_consistency(module, ignore_regex=r'.*\.w_avg')
                    module = copy.deepcopy(module).eval().requires_grad_(False).cpu()
                snapshot_data[name] = module
                del module      # conserve memory
            snapshot_pkl = os.path.join(run_dir, f'network-snapshot-{cur_nimg//1000:06d}.pkl')
            if rank == 0:
                with open(snapshot_pkl, 'wb') as f:
                    pickle.dump(snapshot_data, f)
            del snapshot_data

        # Evaluate metrics (:604-614): every rank computes, rank 0 reports.
        if (snapshot_pkl is not None) and metrics:
            from metrics import metric_main
            if rank == 0:
                print('Evaluating metrics...')
            for metric in metrics:
                result_dict = metric_main.calc_metric(metric=metric, G=G_ema, num_gpus=num_gpus, rank=rank, device=device,
                                                      dataset_kwargs=metric_set_kwargs if metric_set_kwargs is not None else training_set_kwargs)
                if rank == 0:
                    metric_main.report_metric(result_dict, run_dir=run_dir, snapshot_pkl=snapshot_pkl)
                stats_metrics.update(result_dict.results)

        # Collect statistics.
        for phase in step.phases:
            value = []
            if (phase.start_event is not None) and (phase.end_event is not None) and step.batch_idx > 0 and phase.timed:
                phase.end_event.synchronize()
                value = phase.start_event.elapsed_time(phase.end_event)
            report0('Timing/' + phase.name, value)
        stats_collector.update()
        stats_dict = stats_collector.as_dict()

        # Update logs.
        timestamp = time.time()
        if stats_jsonl is not None:
            stats_jsonl.write(json.dumps(dict(stats_dict, timestamp=timestamp)) + '\n')
            stats_jsonl.flush()
        if stats_tfevents is not None:
            global_step = int(cur_nimg / 1e3)
            walltime = timestamp - start_time
            for name, value in stats_dict.items():
                stats_tfevents.add_scalar(name, value.mean, global_step=global_step, walltime=walltime)
            for name, value in stats_metrics.items():
                stats_tfevents.add_scalar(f'Metrics/{name}', value, global_step=global_step, walltime=walltime)
            stats_tfevents.flush()
        if progress_fn is not None:
            progress_fn(cur_nimg // 1000, total_kimg)

        # Update state.
        cur_tick += 1
        tick_start_nimg = cur_nimg

        # Save the training state: the last act of the tick's maintenance, so that the next thing that happens is step.run.
        if save_state and snapshot_pkl is not None:
            extras = dict(cur_tick=cur_tick, elapsed_sec=time.time() - start_time, random_seed=int(random_seed), options=options_json)
            if rank == 0:
                extras['grid_z'] = torch.cat(step.grid_z)
            state_pt = os.path.join(run_dir, f'training-state-{cur_nimg//1000:06d}.pt')
            if train_state.save_state(state_pt, step, extras) is not None:
                for _, older in train_state.state_files(run_dir):
                    if os.path.abspath(older) != os.path.abspath(state_pt):
                        os.remove(older)
            if num_gpus > 1:        # nobody goes on (or returns, to read the file) before rank 0 has written it
                written = torch.zeros([1], device=device)
                torch.distributed.all_reduce(written)
                written.item()
        tick_start_time = time.time()
        maintenance_time = tick_start_time - tick_end_time
        if done:
            break

    if stats_jsonl is not None:
        stats_jsonl.close()
    if rank == 0:
        print()
        print('Exiting...')
    return step

#----------------------------------------------------------------------------
