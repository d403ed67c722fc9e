"""The body-part geometry's second rule without a GPU: tests/part_geometry_ref.py, the restatement of
csrc/part_geometry.hip, against the host's part_quadrilateral / part_matrices; ``patch_pipeline.part_valid``; and the
``--part-geometry`` option of the three command lines."""
import json
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import part_geometry_ref as ref
from oracle.ref_patches import source_coordinates
from train_grid_tree import make_tree
from training import patch_pipeline

CASES = [(256, 32, False), (256, 0, True), (512, 0, False), (512, 32, True)]       # height, x_pad, shin_fallback


def _people(size):
    return np.concatenate([ref.edge_people(size)[0], ref.standing_people(6, size, seed=size)])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize('height,x_pad,shin', CASES)
def test_the_restated_quadrilaterals_are_the_hosts_bit_for_bit(height, x_pad, shin):
    people, seen_none, seen_fallback = _people(height), 0, 0
    for kp in people:
        for k, part in enumerate(patch_pipeline.BODY_PARTS):
            want = patch_pipeline.part_quadrilateral(kp, part, height, x_pad=x_pad, shin_fallback=shin)
            got = ref.quadrilateral(kp, k, height, x_pad, shin)
            assert (want is None) == (got is None), (k, kp)
            if want is None:
                seen_none += 1
                continue
            assert want.dtype == np.float32 and got.dtype == np.float32 and np.array_equal(_bits(want), _bits(got)), (k, want, got)
            seen_fallback += not patch_pipeline._seen(kp, part)
    assert seen_none >= 10 and seen_fallback >= 4          # the people do reach the missing parts and the fall-backs


@pytest.mark.parametrize('height,x_pad,shin', CASES)
def test_part_valid_is_part_matrices_flags(height, x_pad, shin):
    people = _people(height)
    want = patch_pipeline.part_matrices(people, height, height, x_pad=x_pad, shin_fallback=shin)[2]
    got = patch_pipeline.part_valid(people, shin_fallback=shin)
    assert got.dtype == bool and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(ref.part_matrices(people, height, height, x_pad=x_pad, shin_fallback=shin)[2], want)
    assert want.any(axis=0).all() and not want.all(axis=0).any()        # every part is there for someone and missing for someone


def test_the_confidence_edges():
    people, names = ref.edge_people(256)
    at, below = people[names.index('confidence exactly 0.1')], people[names.index('confidence just below 0.1')]
    assert at[ref.LELB, 2] == 0.1 and below[ref.LELB, 2] < 0.1 and np.float32(below[ref.LELB, 2]) == np.float32(0.1)
    valid = patch_pipeline.part_valid(np.stack([at, below]))
    assert valid[0, 2] and valid[0, 3] and not valid[1, 2] and not valid[1, 3]     # the comparison is the host's, in float64


@pytest.mark.parametrize('size', [256, 512])
def test_against_lapack_on_sixty_people(size):
    """Every fixed-point source coordinate (1/32 pixel) of every forward map (patch-sized destination) and every back map
    (image-sized destination) of 60 seeded standing people, the restatement against the host's LAPACK solve: none differs by more
    than one unit, and at most 1e-5 of them differ at all.  (Seen: 13 of 83,558,400 coordinates at 256, 78 of 334,233,600 at 512.)"""
    people = ref.standing_people(60, size, seed=1000 + size)
    host = patch_pipeline.part_matrices(people, size, size, x_pad=0)
    mine = ref.part_matrices(people, size, size, x_pad=0)
    assert np.array_equal(host[2], mine[2]) and host[2].all()
    scale = np.abs(host[0]).max(axis=(2, 3), keepdims=True)
    assert (np.abs(mine[0] - host[0]) <= 1e-11 * scale).all()              # the matrices themselves: the same solution
    total = differ = worst = 0
    for i in range(len(people)):
        for k in range(10):
            for direction, (w, h) in ((0, (size // 4, size // 4)), (1, (size, size))):
                inv_a = patch_pipeline.adjugate_inverse(host[direction][i, k])
                inv_b = np.reshape(ref.inverse(list(mine[direction][i, k].reshape(-1))), [3, 3])
                if np.array_equal(_bits(inv_a), _bits(inv_b)):             # the same bits in: the same 2 w h coordinates out
                    total += 2 * w * h
                    continue
                a, b = source_coordinates(inv_a, w, h), source_coordinates(inv_b, w, h)
                for x, y in zip(a, b):
                    d = np.abs(x - y)
                    total, differ, worst = total + d.size, differ + int(np.count_nonzero(d)), max(worst, int(d.max()))
    print('part geometry against LAPACK at %d: %d of %d coordinates differ, by at most %d' % (size, differ, total, worst))
    assert worst <= 1
    assert differ <= 1e-5 * total


def test_a_zero_length_forearm_is_a_singular_forward_system():
    people, names = ref.edge_people(512)
    kp = people[names.index('zero-length right forearm')][None]
    host, mine = patch_pipeline.part_matrices(kp, 512, 512, x_pad=0), ref.part_matrices(kp, 512, 512, x_pad=0)
    unit = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1.0]).reshape(3, 3)
    assert host[2][0, 5] and mine[2][0, 5]                                  # the part stays valid
    assert np.array_equal(host[0][0, 5], unit) and np.array_equal(mine[0][0, 5], unit)
    g = ref.geometry(kp, 512, 128, 128, 0, False)
    assert not g['fwd_inv'][0, 5].any() and g['valid'][0, 5] == 1


# ---- the option ----

TRAIN = ('--cfg', 'fashion', '--batch', '4', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('part_geometry_cli'))


def _options(output):
    return json.loads(output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')])


def _train(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_the_training_command_records_the_option_only_when_gpu(tree, tmp_path):
    plain, host, gpu = (_train(tree, tmp_path / 'runs', *TRAIN, *extra) for extra in ((), ('--part-geometry', 'host'), ('--part-geometry', 'gpu')))
    assert plain.exit_code == 0 and host.exit_code == 0 and gpu.exit_code == 0, (plain.output, host.output, gpu.output)
    assert host.output == plain.output and 'part_geometry' not in plain.output.replace('part_geometry_cli', '') and 'Part geometry' not in plain.output
    a, b = _options(plain.output), _options(gpu.output)
    assert b.pop('part_geometry') == 'gpu' and b['run_dir'].endswith('-geomgpu') and 'Part geometry:      gpu' in gpu.output
    b['run_dir'] = b['run_dir'][:-len('-geomgpu')]
    assert a == b                                                           # nothing else moved
    both = _train(tree, tmp_path / 'runs', *TRAIN, '--part-geometry', 'gpu', '--swap_weight', '1')
    assert both.exit_code == 0 and _options(both.output)['run_dir'].endswith('-swap1-geomgpu')


def test_an_unknown_value_is_a_usage_error_in_all_three_commands(tree, tmp_path):
    import test as test_256
    import test_512
    res = _train(tree, tmp_path / 'runs', *TRAIN, '--part-geometry', 'fpga')
    assert res.exit_code == 2 and '--part-geometry' in res.output, res.output
    for command in (test_256.generate_images, test_512.generate_images):
        res = CliRunner().invoke(command, ['--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', tree,
                                           '--part-geometry', 'fpga'])
        assert res.exit_code == 2 and '--part-geometry' in res.output and 'fpga' in res.output, res.output
        option, = [p for p in command.params if p.name == 'part_geometry']
        assert option.default == 'host' and list(option.type.choices) == ['host', 'gpu']
    assert not (tmp_path / 'out').exists() and not (tmp_path / 'runs').exists()
    from training.tryon_batch import FullBodyBatchBuilder
    with pytest.raises(ValueError, match='part geometry'):
        FullBodyBatchBuilder('cpu', geometry='fpga')
    import train_wo_flow_fullbody as T
    with pytest.raises(T.UserError, match='--part-geometry'):
        T.setup_training_loop_kwargs(data=tree, cfg='fashion', part_geometry='fpga')


def test_continue_keeps_the_recorded_value(tree, tmp_path):
    from training import train_state
    import train_wo_flow_fullbody as T
    res = _train(tree, tmp_path / 'runs', *TRAIN, '--part-geometry', 'gpu')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=4, batch_gpu=4, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    for value in ('gpu', 'host'):
        res = _train(tree, tmp_path / 'out', '--continue', str(run_dir), '--part-geometry', value)
        assert res.exit_code != 0 and '--part-geometry cannot be given with --continue' in res.output, res.output
    res = _train(tree, tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    assert _options(res.output)['part_geometry'] == 'gpu' and 'Part geometry:      gpu' in res.output
    assert 'part_geometry' not in T.CONTINUE_MAY_CHANGE
