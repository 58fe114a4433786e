"""--replay on the device: the training loop through ONE recording of the step, read from a static batch slot, against the
same loop with the step launched eagerly (replay_eager) -- bit for bit in the deterministic mode; the slot's contents; the
equivalence of padding every caption batch to WORDS_NUM; the fallback; the entry points.

The toy directory is written here: 8 training images in 2 classes (every batch of 4 holds a same-class pair, so the
same-class mask of the DAMSM losses is never all zero and differs from batch to batch) and captions of 3 to 8 words
(some batches are shorter than WORDS_NUM = 8, and the padding masks differ from batch to batch)."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WORDS = ['bird', 'red', 'small', 'wing', 'blue', 'beak', 'long', 'white', 'yellow', 'belly', 'tail', 'black']
# words per caption, two captions per training image: images 0 and 5 fill the WORDS_NUM = 8 columns, the others do not
LENGTHS = [(8, 8), (3, 5), (4, 4), (6, 3), (5, 7), (8, 7), (3, 3), (4, 6)]
CLASSES = [1, 1, 1, 1, 2, 2, 2, 2]
B, WORDS_NUM, CROP, SEED, STEPS = 4, 8, 128, 3, 5


def make_dataset(root):
    """a CUB-shaped toy data_dir with its own class_info.pickle: 8 training images in 2 classes"""
    from PIL import Image
    rng = np.random.RandomState(0)
    for sub in ('images/cls', 'text/cls', 'train', 'test'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    names = {'train': ['cls/a%d' % i for i in range(8)], 'test': ['cls/t0', 'cls/t1']}
    lengths = {'train': LENGTHS, 'test': [(4, 5), (3, 6)]}
    classes = {'train': CLASSES, 'test': [1, 2]}
    for split, keys in names.items():
        with open(os.path.join(root, split, 'filenames.pickle'), 'wb') as f:
            pickle.dump(keys, f)
        with open(os.path.join(root, split, 'class_info.pickle'), 'wb') as f:
            pickle.dump(classes[split], f)
        for k, lens in zip(keys, lengths[split]):
            Image.fromarray(rng.randint(0, 255, (90, 110, 3)).astype(np.uint8)).save(
                os.path.join(root, 'images', k + '.jpg'))
            with open(os.path.join(root, 'text', k + '.txt'), 'w') as f:
                for n in lens:
                    f.write(' '.join(WORDS[rng.randint(0, len(WORDS))] for _ in range(n)) + '\n')
    return root


def toy_cfg():
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 2
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.TEXT.EMBEDDING_DIM = 2, WORDS_NUM, 256
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL = B, 3, 1
    cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.CUDA, cfg.GPU_ID = '', '', True, True, 0
    s = cfg.TRAIN.SMOOTH
    s.GAMMA1, s.GAMMA2, s.GAMMA3, s.LAMBDA = 4.0, 5.0, 10.0, 5.0
    return cfg


def host_masks(d):
    """(class mask, word mask) of one batch's draws, by the definitions written out"""
    ids = np.asarray(d.class_ids, dtype=np.int64)
    cm = np.array([[1 if (ids[j] == ids[i] and j != i) else 0 for j in range(len(ids))] for i in range(len(ids))],
                  dtype=np.uint8)
    return cm, (np.asarray(d.captions).reshape(len(ids), -1) == 0)


def run_draws(loader, steps):
    """the draws of the first `steps` batches a loader with this seed will make (host only: no launch)"""
    out = []
    while len(out) < steps:
        for indices in loader.epoch_indices():
            out.append(loader.draw_batch(indices))
            if len(out) == steps:
                break
    return out


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    from sbagan.device_data import DeviceImageCache
    toy_cfg()
    root = make_dataset(str(tmp_path_factory.mktemp('replay') / 'toy'))
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    cache = DeviceImageCache(ds, int(CROP * 76 / 64), torch.device('cuda', 0), max_bytes=1 << 30, workers=0)
    return {'root': root, 'ds': ds, 'cache': cache, 'tmp': tmp_path_factory, 'runs': {}}


@pytest.fixture()
def det():
    from miscc.config import reset_cfg
    from sbagan import ops
    toy_cfg()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)
    reset_cfg()


def make_loader(toy):
    from sbagan.device_data import DeviceBatchLoader
    return DeviceBatchLoader(toy['ds'], toy['cache'], B, CROP, 2, seed=SEED)


def test_the_toy_run_has_batches_that_differ(toy, det):
    """a condition on the INPUTS of the runs below, checked on the host from the loader's draws"""
    draws = run_draws(make_loader(toy), STEPS)
    masks = [host_masks(d) for d in draws]
    assert all(cm.any() for cm, _ in masks)                                     # a same-class pair in every batch
    assert any(not np.array_equal(masks[0][0], cm) for cm, _ in masks[1:])      # class masks differ
    assert any(not np.array_equal(masks[0][1], wm) for _, wm in masks[1:])      # word masks differ
    longest = [int(d.lengths.max()) for d in draws]
    assert min(longest) < WORDS_NUM and max(longest) == WORDS_NUM, longest


def trained(toy, dtype, eager, interval=1000, steps=STEPS):
    """one --device_data --replay run of the trainer (cached per arguments): the final training state, the checkpoint
    files, and what the slot and the loader held at the end"""
    key = (str(dtype), bool(eager), interval, steps)
    if key in toy['runs']:
        return toy['runs'][key]
    from sbagan import ops
    from trainer import condGANTrainer
    ops.set_compute_dtype(dtype)
    ds, loader = toy['ds'], make_loader(toy)
    out_dir = str(toy['tmp'].mktemp('out'))
    torch.manual_seed(3)
    algo = condGANTrainer(out_dir, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.replay, algo.replay_eager, algo.average_interval = True, eager, interval
    algo.train(max_steps=steps)
    torch.cuda.synchronize()
    gan, state = algo.gan, {}
    for name, flat, opt in [('G', gan.flatG, gan.optG)] + [('D%d' % i, f, o) for i, (f, o) in
                                                            enumerate(zip(gan.flatD, gan.optD))]:
        state[name + '/param'], state[name + '/m'], state[name + '/v'] = flat.data.cpu(), flat.m.cpu(), flat.v.cpu()
        state[name + '/adam_state'] = opt.state.cpu()
        if flat.avg is not None:
            state[name + '/ema'] = flat.avg.cpu()
    files = {}
    for path in sorted(glob.glob(os.path.join(out_dir, 'Model', '*.pth'))):
        files[os.path.basename(path)] = torch.load(path, map_location='cpu')
    slot = algo.slot
    res = {'state': state, 'files': files, 'out_dir': out_dir, 'draws': loader.last_draws,
           'recorded': algo.slot_step.recording is not None,
           'slot': {'mask': slot.mask.cpu(), 'class_mask': slot.class_mask.tensor.cpu(), 'captions': slot.captions.cpu(),
                    'cap_lens': slot.cap_lens.cpu(), 'class_ids': slot.class_ids.cpu(),
                    'imgs': [i.cpu() for i in slot.imgs]}}
    toy['runs'][key] = res
    return res


def assert_same_training(a, b):
    assert sorted(a['files']) == sorted(b['files'])
    assert {'netD0.pth', 'netD1.pth'} <= set(a['files'])
    assert {'netG_epoch_%d.pth' % e for e in range(4)} <= set(a['files'])
    for name in a['files']:
        sa, sb = a['files'][name], b['files'][name]
        assert sorted(sa) == sorted(sb)
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, (name, bad[:5], len(bad))
    bad = [k for k in a['state'] if not torch.equal(a['state'][k], b['state'][k])]
    assert not bad, bad
    for t in a['state'].values():
        assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_replayed_loop_trains_what_the_eager_loop_trains(toy, det, dtype):
    """5 iterations over 3 epochs (2 batches each) and the save_model calls between them: every checkpoint written, the
    generator's parameters, its EMA shadow and every network's Adam moments are torch.equal between the loop over the
    recording and the same loop with eager steps"""
    a, b = trained(toy, dtype, eager=False), trained(toy, dtype, eager=True)
    assert a['recorded'] and not b['recorded']          # (no silent fallback: the first run did go through the recording)
    assert_same_training(a, b)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_average_dump_does_not_disturb_training(toy, det, dtype):
    """the EMA weights are loaded into the generator for the 'average' dump (every 2 iterations here) and put back: the
    recording must read the training weights again afterwards"""
    a, b = trained(toy, dtype, eager=False, interval=2), trained(toy, dtype, eager=True, interval=2)
    assert a['recorded'] and not b['recorded']
    assert_same_training(a, b)
    for r in (a, b):
        assert glob.glob(os.path.join(r['out_dir'], 'Image', 'G_average_*'))
    # the dump itself trains nothing: the run without it ends in the same state
    assert_same_training(a, trained(toy, dtype, eager=False))


def test_after_a_replay_the_slot_holds_this_batch(toy, det):
    from miscc import losses
    from sbagan import ops
    from sbagan.trainer import build_mask
    r = trained(toy, torch.bfloat16, eager=False)
    d, s = r['draws'], r['slot']
    dev = toy['cache'].device
    captions = torch.from_numpy(np.asarray(d.captions).reshape(B, -1))
    assert torch.equal(s['captions'], captions)
    assert s['cap_lens'].tolist() == d.lengths.tolist() and s['class_ids'].tolist() == list(d.class_ids)
    assert torch.equal(s['mask'], build_mask(captions, WORDS_NUM))
    assert torch.equal(s['class_mask'], losses.class_mask(np.asarray(d.class_ids), B, torch.device('cpu')))
    cm, wm = host_masks(d)
    assert np.array_equal(s['class_mask'].numpy(), cm) and np.array_equal(s['mask'].numpy(), wm) and cm.any()
    want = ops.batch_pyramid(toy['cache'], d.params(), CROP, 2)
    for k in range(2):
        assert torch.equal(s['imgs'][k], want[::-1][k].cpu()), 'scale %d' % k
    assert want[0].device == dev


def test_padding_to_words_num_is_equivalent(toy, det):
    """one GANStep (f32), one batch whose longest caption is shorter than WORDS_NUM, the same noise and eps from the same
    state: the step with words_embs / mask as wide as max(cap_lens) and the step at WORDS_NUM agree in every loss within
    the project's parity bar for losses, 1e-3 relative.  (Measured on an MI355X: every entry bit-identical, difference 0.)"""
    from sbagan import ops
    from sbagan.static_batch import StaticBatch
    from sbagan.trainer import build_mask
    from trainer import condGANTrainer
    from miscc.config import cfg
    ops.set_compute_dtype(torch.float32)
    ds, loader = toy['ds'], make_loader(toy)
    dev = toy['cache'].device
    torch.manual_seed(3)
    algo = condGANTrainer(str(toy['tmp'].mktemp('pad')), loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    text_encoder, image_encoder, netG, netsD, _ = algo.build_models()
    algo.define_optimizers(netG, netsD, image_encoder)
    netG.set_return_attention(False)
    gan = algo.gan
    batch = None
    for _ in range(3):
        for batch in loader:
            if int(loader.last_draws.lengths.max()) < WORDS_NUM:
                break
        else:
            continue
        break
    longest = int(loader.last_draws.lengths.max())
    assert longest < WORDS_NUM
    imgs, captions, cap_lens, class_ids, keys = batch
    slot = StaticBatch(B, WORDS_NUM, 2, CROP, dev)
    slot.load(batch)
    slot.prologue(text_encoder, encode=algo._encode)()
    noise = torch.randn((B, cfg.GAN.Z_DIM), device=dev)
    eps = torch.randn((B, cfg.GAN.CONDITION_DIM), device=dev)
    snap = gan.snapshot()
    words, sent = algo._encode(text_encoder, captions, cap_lens)
    assert words.size(2) == longest and slot.words_embs.size(2) == WORDS_NUM
    narrow = gan.step(imgs, sent, words, build_mask(captions, longest), cap_lens, slot.class_mask, noise, eps=eps)
    narrow = {k: float(v) for k, v in narrow.items()}
    gan.restore(snap)
    wide = gan.step(slot.imgs, slot.sent_emb, slot.words_embs, slot.mask, slot.cap_lens, slot.class_mask, noise, eps=eps)
    wide = {k: float(v) for k, v in wide.items()}
    assert sorted(narrow) == sorted(wide) and len(narrow) >= 8
    rel = {k: abs(wide[k] - narrow[k]) / max(abs(narrow[k]), 1e-30) for k in narrow}
    print('padding to WORDS_NUM, relative loss differences:', {k: '%.3g' % v for k, v in sorted(rel.items())})
    for k in narrow:
        assert np.isfinite(narrow[k]) and np.isfinite(wide[k])
        assert rel[k] <= 1e-3, (k, narrow[k], wide[k])


def test_fallback_when_the_recording_cannot_be_made(toy, det, monkeypatch, capsys):
    """a Python exception at the construction of the recording: one line, and the run goes on with eager steps"""
    import sbagan.trainer as st

    def refuse(self, *a, **kw):
        raise RuntimeError('no recording today')
    monkeypatch.setattr(st.ReplayedStep, '__init__', refuse)
    r = trained(toy, torch.bfloat16, eager=False, steps=3)
    text = capsys.readouterr().out
    assert text.count('--replay: the step could not be recorded') == 1 and 'no recording today' in text
    assert not r['recorded']
    assert {'netD0.pth', 'netD1.pth', 'netG_epoch_3.pth'} <= set(r['files'])
    for sd in r['files'].values():
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    del toy['runs'][(str(torch.bfloat16), False, 1000, 3)]          # (not a recorded run: nobody else may reuse it)


def _yml(tmp_path, root, **train):
    import yaml
    t = {'FLAG': True, 'NET_E': '', 'NET_G': '', 'BATCH_SIZE': B, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1}
    t.update(train)
    yml = tmp_path / 'toy.yml'
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'toy', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'TREE': {'BRANCH_NUM': 2, 'BASE_SIZE': 64}, 'TRAIN': t, 'GAN': {'GF_DIM': 32, 'DF_DIM': 64},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': WORDS_NUM}}))
    return str(yml)


def _checkpoints(tmp_path):
    """the Model directory of the one run whose output went to <tmp_path>/output/"""
    dirs = glob.glob(os.path.join(str(tmp_path), 'output', '*', 'Model'))
    assert len(dirs) == 1, dirs
    files = {os.path.basename(p): torch.load(p, map_location='cpu') for p in glob.glob(os.path.join(dirs[0], '*.pth'))}
    assert {'netG_epoch_1.pth', 'netD0.pth', 'netD1.pth'} <= set(files)
    for sd in files.values():
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    return files


def test_entry_point_hands_the_flag_over_and_trains_from_the_torch_loader(toy, tmp_path, monkeypatch):
    import main
    from miscc.config import reset_cfg
    from sbagan import device_data, ops
    from trainer import condGANTrainer
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    yml = _yml(tmp_path, toy['root'])
    (tmp_path / 'cwd').mkdir()
    monkeypatch.chdir(tmp_path / 'cwd')
    made = []

    class Stub(object):
        def __init__(self, output_dir, dataloader, n_words, ixtoword):
            self.loader = dataloader
            made.append(self)

        def train(self):
            pass

    base = ['--cfg', yml, '--gpu', '0', '--manualSeed', '5']
    main.main(base + ['--device_data', '--device_data_gb', '1', '--replay'], make_trainer=Stub)
    main.main(base + ['--device_data', '--device_data_gb', '1'], make_trainer=Stub)
    assert made[0].replay is True and isinstance(made[0].loader, device_data.DeviceBatchLoader)
    assert made[1].replay is False

    # --replay with the torch DataLoader: 8 images, batches of 4, one epoch = 2 steps through the slot's copy_ path
    trainers = []

    def make(output_dir, dataloader, n_words, ixtoword):
        trainers.append(condGANTrainer(output_dir, dataloader, n_words, ixtoword, allow_random_encoders=True))
        return trainers[-1]

    main.main(base + ['--replay'], make_trainer=make)
    assert type(trainers[0].data_loader) is torch.utils.data.DataLoader
    assert trainers[0].replay is True and trainers[0].slot is not None
    _checkpoints(tmp_path)
    reset_cfg()


def test_main_bert_with_replay_and_mixing(toy, tmp_path, monkeypatch):
    """main_bert.main --replay with TRAIN.MIXING: 2 steps, the step's static noise is 2 x B x nz"""
    import main_bert
    import model_bert
    import trainer_bert
    from miscc.config import cfg, reset_cfg
    from sbagan import ops
    from test_bert_entry_gpu import _bert_dir
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    yml = _yml(tmp_path, toy['root'], MIXING=True)
    (tmp_path / 'cwd').mkdir()
    monkeypatch.chdir(tmp_path / 'cwd')
    made = []

    make = trainer_bert.condGANTrainer.__init__

    def make_random(self, *a, **kw):        # (the entry point has no switch for randomly initialised encoders)
        kw['allow_random_encoders'] = True
        make(self, *a, **kw)
        made.append(self)

    monkeypatch.setattr(trainer_bert.condGANTrainer, '__init__', make_random)
    main_bert.main(['--cfg', yml, '--gpu', '0', '--manualSeed', '5', '--replay', '--bert_dir', _bert_dir(tmp_path)])
    algo = made[0]
    assert algo.replay is True and cfg.TRAIN.MIXING and type(algo.gan.netG) is model_bert.G_NET_MIX
    assert algo._noise_shape(B) == (2, B, cfg.GAN.Z_DIM)
    _checkpoints(tmp_path)
    reset_cfg()
