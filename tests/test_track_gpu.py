"""--track on the device: the invariants of sbagan/track.py, bit for bit in the deterministic-reduction mode.

The toy directory is written here: 4 training images in 2 classes (2 batches of 2 an epoch, 3 epochs) and 6 held-out
images in 3 classes with captions of 3 to 8 words.  --track_n 5 with batches of 2 leaves a short last batch.  Every
training run is made once per module and shared by the tests that read it."""
import glob
import json
import os
import pickle
import random

import numpy as np
import pytest
import torch

from test_replay_train_gpu import WORDS, assert_same_training

pytestmark = pytest.mark.gpu

B, WORDS_NUM, CROP, SEED, EPOCHS = 2, 8, 128, 3, 3
TRAIN_CLASSES, TEST_CLASSES = [1, 1, 2, 2], [1, 2, 3, 1, 2, 3]
TRAIN_LENGTHS = [(8, 5), (3, 6), (4, 4), (7, 3)]
TEST_LENGTHS = [(8, 4), (3, 5), (6, 6), (5, 8), (4, 3), (7, 5)]
EVALUATORS = dict(kid=True, kid_subsets=4, kid_subset_size=4, prdc=2, r_precision=3)
POLICY = 'color,translation,cutout'


def make_dataset(root):
    from PIL import Image
    rng = np.random.RandomState(1)
    for sub in ('images/cls', 'text/cls', 'train', 'test'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    names = {'train': ['cls/a%d' % i for i in range(4)], 'test': ['cls/t%d' % i for i in range(6)]}
    lengths = {'train': TRAIN_LENGTHS, 'test': TEST_LENGTHS}
    classes = {'train': TRAIN_CLASSES, 'test': TEST_CLASSES}
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


def toy_cfg(max_epoch=EPOCHS):
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 2
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.TEXT.EMBEDDING_DIM = 2, WORDS_NUM, 256
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL = B, max_epoch, 1
    cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.CUDA, cfg.GPU_ID = '', '', True, True, 0
    s = cfg.TRAIN.SMOOTH
    s.GAMMA1, s.GAMMA2, s.GAMMA3, s.LAMBDA = 4.0, 5.0, 10.0, 5.0
    return cfg


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    from miscc import transforms
    from sbagan.device_data import DeviceImageCache
    toy_cfg()
    root = make_dataset(str(tmp_path_factory.mktemp('track') / 'toy'))
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    tfm = transforms.Compose([transforms.Resize(int(CROP * 76 / 64)), transforms.RandomCrop(CROP),
                              transforms.RandomHorizontalFlip()])
    ds_host = datasets.TextDataset(root, 'train', base_size=64, transform=tfm)
    cache = DeviceImageCache(ds, int(CROP * 76 / 64), torch.device('cuda', 0), max_bytes=1 << 30, workers=0)
    made = {}

    def ds_bert():
        """(the training split as datasets_bert reads it, the toy BERT directory), made at the first call"""
        if not made:
            import datasets_bert
            from test_bert_entry_gpu import _bert_dir
            bert_dir = _bert_dir(tmp_path_factory.mktemp('bert'))
            made['v'] = (datasets_bert.TextDataset(root, 'train', base_size=64, transform=tfm, bert_dir=bert_dir), bert_dir)
        return made['v']
    return {'root': root, 'ds': ds, 'ds_host': ds_host, 'ds_bert': ds_bert, 'cache': cache, 'tmp': tmp_path_factory,
            'runs': {}}


@pytest.fixture()
def det():
    from miscc.config import reset_cfg
    from sbagan import ops
    toy_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)
    reset_cfg()


def generator_states():
    return random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()


def same_generator_states(a, b):
    return (a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]
            and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]))


def trained(toy, mode, track=0, n=5, best=None, fid=False, fused=False, ada=False, max_epoch=EPOCHS, captions=1,
            snapshot=1):
    """one training run of the trainer (cached per arguments).  mode: 'eager' (the plain loop over the torch DataLoader),
    'replay' (the recording, device loader), 'replay_eager' (the same loop, eager steps), 'replay_host' (the recording
    fed by the torch DataLoader: --replay without --device_data) or 'bert' (the BERT trainer, plain loop)"""
    key = (mode, track, n, best, fid, fused, ada, max_epoch, captions, snapshot)
    if key in toy['runs']:
        return toy['runs'][key]
    from miscc.config import cfg
    from sbagan.device_data import DeviceBatchLoader
    from trainer import condGANTrainer
    toy_cfg(max_epoch)
    cfg.TRAIN.SNAPSHOT_INTERVAL = snapshot
    if mode == 'bert':
        toy['ds_bert']()        # (made at the first call, with draws of its own: ahead of the seeding)
    for seeder in (random.seed, np.random.seed, torch.manual_seed, torch.cuda.manual_seed_all):
        seeder(SEED)
    make = lambda *a: condGANTrainer(*a, allow_random_encoders=True)
    if mode == 'bert':
        import trainer_bert
        ds, bert_dir = toy['ds_bert']()
        make = lambda *a: trainer_bert.condGANTrainer(*a, allow_random_encoders=True, bert_dir=bert_dir)
    if mode == 'bert':
        loader = torch.utils.data.DataLoader(ds, batch_size=B, drop_last=True, shuffle=True, num_workers=0)
    elif mode in ('eager', 'replay_host'):
        ds = toy['ds_host']
        loader = torch.utils.data.DataLoader(ds, batch_size=B, drop_last=True, shuffle=True, num_workers=0)
    else:
        ds = toy['ds']
        loader = DeviceBatchLoader(ds, toy['cache'], B, CROP, 2, seed=SEED)
    out_dir = str(toy['tmp'].mktemp('out'))
    algo = make(out_dir, loader, ds.n_words, ds.ixtoword)
    algo.replay, algo.replay_eager = mode.startswith('replay'), mode == 'replay_eager'
    algo.track_captions = captions
    for name, value in EVALUATORS.items():
        setattr(algo, name, value)
    algo.fid, algo.fused_inference = fid, fused
    algo.track, algo.track_n, algo.track_best = track, n, best
    if ada:
        # (p starts in the middle and travels 0.4 per controller update: it moves within these few steps)
        algo.diffaug, algo.ada, algo.ada_kimg, algo.diffaug_p = POLICY, 0.6, 0.02, 0.5
    algo.train()
    torch.cuda.synchronize()
    rng = generator_states()
    gan, state = algo.gan, {}
    for name, flat, opt in [('G', gan.flatG, gan.optG)] + [('D%d' % i, f, o) for i, (f, o) in
                                                            enumerate(zip(gan.flatD, gan.optD))]:
        state[name + '/param'], state[name + '/m'], state[name + '/v'] = flat.data.cpu(), flat.m.cpu(), flat.v.cpu()
        state[name + '/adam_state'] = opt.state.cpu()
        if flat.avg is not None:
            state[name + '/ema'] = flat.avg.cpu()
    for name, buf in gan.netG.named_buffers():                        # the BatchNorm running statistics
        state['G/buffer/' + name] = buf.detach().cpu().clone()
    for i, d in enumerate(gan.netsD):
        for name, buf in d.named_buffers():
            state['D%d/buffer/%s' % (i, name)] = buf.detach().cpu().clone()
    model_dir = os.path.join(out_dir, 'Model')
    files = {os.path.basename(p): torch.load(p, map_location='cpu')
             for p in sorted(glob.glob(os.path.join(model_dir, '*.pth'))) if os.path.basename(p) != 'netG_best.pth'}
    jsonl = os.path.join(model_dir, 'track.jsonl')
    records = [json.loads(line) for line in open(jsonl)] if os.path.exists(jsonl) else None
    res = {'state': state, 'files': files, 'model_dir': model_dir, 'rng': rng, 'records': records, 'algo': algo,
           'recorded': algo.slot_step is not None and algo.slot_step.recording is not None,
           'ada': gan.augment.state_dict() if gan.augment is not None else None}
    toy['runs'][key] = res
    return res


def without_seconds(records):
    out = []
    for r in records:
        assert r['seconds'] > 0
        out.append({k: v for k, v in r.items() if k != 'seconds'})
    return out


def assert_undisturbed(tracked, plain):
    assert plain['records'] is None and len(tracked['records']) == EPOCHS + 1
    assert_same_training(tracked, plain)
    assert same_generator_states(tracked['rng'], plain['rng'])
    assert any(k.startswith('G/buffer/') and k.endswith('running_mean') for k in plain['state'])


# ------------------------------------------------------------------ 1. training is untouched
def test_eager_training_is_undisturbed(toy, det):
    """3 epochs of 2 batches from the shuffled torch DataLoader, --track 1 against the same run without it: every
    checkpoint, parameter, EMA shadow, Adam moment and running statistic, and the python / numpy / torch generator states"""
    assert_undisturbed(trained(toy, 'eager', track=1), trained(toy, 'eager'))


def test_replayed_training_is_undisturbed(toy, det):
    a, b = trained(toy, 'replay', track=1, best='kid.kid'), trained(toy, 'replay')
    assert a['recorded'] and b['recorded']
    assert_undisturbed(a, b)


def test_training_with_ada_is_undisturbed(toy, det):
    a, b = trained(toy, 'replay', track=1, ada=True), trained(toy, 'replay', ada=True)
    assert a['recorded'] and b['recorded']
    assert_undisturbed(a, b)
    assert 'ada_state.pth' in a['files'] and sorted(a['ada']) == ['counters', 'p', 'rt']
    for name in a['ada']:
        assert torch.equal(a['ada'][name], b['ada'][name]), name
    assert bool((a['ada']['p'] != 0.5).any())                         # (the controller did move p in this run)


# ------------------------------------------------------------------ 2. replay equals eager with tracking on
def test_replayed_loop_with_tracking_equals_the_eager_loop_with_tracking(toy, det):
    a, b = trained(toy, 'replay', track=1, best='kid.kid'), trained(toy, 'replay_eager', track=1, best='kid.kid')
    assert a['recorded'] and not b['recorded']
    assert_same_training(a, b)
    assert without_seconds(a['records']) == without_seconds(b['records'])


# ------------------------------------------------------------------ 3. the schedule
def test_records_are_those_the_schedule_names(toy, det):
    from sbagan.track import due
    one, two = trained(toy, 'replay', track=1, best='kid.kid'), trained(toy, 'replay', track=2)
    for run, every in ((one, 1), (two, 2)):
        assert [r['epoch'] for r in run['records']] == [e for e in range(EPOCHS) if due(e, every)] + [EPOCHS]
        for r in run['records']:
            assert (r['split'], r['images'], r['captions_per_image']) == ('test', 5, 1)
            assert r['checkpoint'] == 'netG_epoch_%d.pth' % r['epoch'] and r['iteration'] == 2 * min(r['epoch'] + 1, EPOCHS)
            assert sorted(r['metrics']) == ['kid', 'prdc', 'r_precision']
            assert r['metrics']['kid']['n_fake'] == r['metrics']['kid']['n_real'] == 5
            assert r['metrics']['r_precision']['n'] == 5 and r['metrics']['prdc']['k'] == 2
    # a record is a function of the weights alone: whether or not epoch 1 was evaluated, epochs 0, 2 and 3 read the same
    shared = {r['epoch']: r for r in without_seconds(one['records'])}
    assert [shared[r['epoch']] for r in without_seconds(two['records'])] == without_seconds(two['records'])
    # the final evaluation reads the weights of the last epoch's once more
    assert shared[EPOCHS]['metrics'] == shared[EPOCHS - 1]['metrics']
    kids = [r['metrics']['kid']['kid'] for r in one['records']]
    assert len(set(kids)) > 1 and all(np.isfinite(kids))               # (the generators of the epochs do differ)


def test_evaluating_the_same_weights_twice_gives_the_same_record(toy, det):
    run = trained(toy, 'replay', track=1, best='kid.kid')
    algo = run['algo']
    netG = algo.gan.netG
    was = netG.training
    netG.eval()
    try:
        first = algo.tracker.measure(netG, netG.ca_net)
        second = algo.tracker.measure(netG, netG.ca_net)
    finally:
        netG.train(was)
    assert json.dumps(first, sort_keys=True) == json.dumps(second, sort_keys=True)


# ------------------------------------------------------------------ 4. a record equals the offline evaluation
def offline(tracker, ckpt, fid, G_NET=None):
    """what the evaluator classes give for a checkpoint loaded afresh, over the tracker's stored captions, noise, eps,
    real rows and pool: the loop written out here, nothing of Tracker.measure"""
    import model
    from sbagan.feature_rows import dtype_name
    from sbagan.fid import FID
    from sbagan.kid import KID
    from sbagan.prdc import PRDC
    from sbagan.rprecision import RPrecision
    dev = tracker.noise.device
    netG = (G_NET or model.G_NET)()
    netG.load_state_dict(torch.load(ckpt, map_location='cpu'))
    netG.to(dev).eval()
    enc = tracker.image_encoder
    ranking = RPrecision(enc, tracker.pool[0], tracker.pool[1], R=3, seed=100)
    prdc = PRDC(enc.pooled_features, D=2048, k=2, dtype=dtype_name())
    kid = KID(enc.pooled_features, D=2048, subsets=4, subset_size=4, seed=100, dtype=dtype_name(), rows=prdc)
    fd = FID(enc.pooled_features, D=2048, dtype=dtype_name()) if fid else None
    rows = [ev for ev in (fd, prdc) if ev is not None]
    from sbagan import ops
    with torch.no_grad():
        for lo in range(0, tracker.rows, B):
            hi = min(lo + B, tracker.rows)
            ops.det_reset()
            netG.ca_net.eps = tracker.eps[lo:hi]
            last = netG(tracker.noise[lo:hi], tracker.sent_emb[lo:hi], tracker.words_embs[lo:hi],
                        tracker.mask[lo:hi])[0][-1]
            ranking.update(last, tracker.sent_emb[lo:hi], tracker.class_ids[lo:hi])
            for ev in rows:
                ev.update_features('fake', enc.last_pooled)
    for ev in rows:
        ev.update_features('real', tracker.real_rows)
    out = {'kid': kid.result(), 'prdc': prdc.result(), 'r_precision': ranking.result()}
    if fid:
        out['fid'] = fd.result()
    return json.loads(json.dumps(out))


def test_a_record_equals_the_offline_evaluation_of_its_checkpoint(toy, det):
    run = trained(toy, 'replay', track=1, best='kid.kid')
    tracker = run['algo'].tracker
    assert tracker.rows == 5 and tracker.slices() == [(0, 2), (2, 4), (4, 5)]          # a short last batch
    assert tracker.class_ids.tolist() == TEST_CLASSES[:5] and tracker.keys == ['cls/t%d' % i for i in range(5)]
    for r in (run['records'][1], run['records'][-1]):
        want = offline(tracker, os.path.join(run['model_dir'], r['checkpoint']), fid=False)
        assert r['metrics'] == want, r['epoch']
        assert 0.0 <= want['r_precision']['r_at_1'] <= 1.0


def test_a_record_with_fid_equals_the_offline_evaluation(toy, det):
    """the one FID case (its host eigensolves take seconds): one epoch, every image of the split"""
    run = trained(toy, 'eager', track=1, n=0, fid=True, max_epoch=1)
    tracker = run['algo'].tracker
    assert [r['epoch'] for r in run['records']] == [0, 1] and tracker.images == 6
    r = run['records'][-1]
    assert sorted(r['metrics']) == ['fid', 'kid', 'prdc', 'r_precision']
    want = offline(tracker, os.path.join(run['model_dir'], r['checkpoint']), fid=True)
    assert r['metrics'] == want
    assert np.isfinite(want['fid']['fid']) and want['fid']['n_real'] == want['fid']['n_fake'] == 6


def test_replay_from_the_torch_loader_is_undisturbed(toy, det):
    """--replay without --device_data: the recording fed by the shuffled torch DataLoader through the slot's copies"""
    a, b = trained(toy, 'replay_host', track=1), trained(toy, 'replay_host')
    assert a['recorded'] and b['recorded']
    assert_undisturbed(a, b)
    c = trained(toy, 'eager', track=1)          # the same loader and seeds, eager steps with their own noise draws:
    assert [r['epoch'] for r in a['records']] == [r['epoch'] for r in c['records']]     # the same schedule


def test_two_captions_per_image(toy, det, capsys):
    """--track_captions 2 over the whole split: 12 generated rows against 6 real ones, rows image-major, and the best
    weights of an epoch that is no snapshot (torch.save of the state dict, the bytes save_model writes)"""
    run = trained(toy, 'eager', track=1, n=0, captions=2, max_epoch=2, snapshot=2)
    tracker, algo = run['algo'].tracker, run['algo']
    assert (tracker.images, tracker.rows) == (6, 12) and tuple(tracker.real_rows.shape) == (6, 2048)
    assert tracker.keys == ['cls/t%d' % (i // 2) for i in range(12)]
    assert tracker.class_ids.tolist() == [TEST_CLASSES[i // 2] for i in range(12)]
    ds = tracker.dataset
    for row in range(12):                                   # caption c of image i is the data set's caption 2 i + c
        want = np.asarray(ds.captions[row][:WORDS_NUM])
        assert tracker.caps[row].tolist() == want.tolist() + [0] * (WORDS_NUM - len(want))
    assert tuple(tracker.words_embs.shape) == (12, 256, WORDS_NUM) and tuple(tracker.mask.shape) == (12, WORDS_NUM)
    assert [(r['epoch'], r['checkpoint']) for r in run['records']] == \
        [(0, 'netG_epoch_0.pth'), (1, None), (2, 'netG_epoch_2.pth')]
    for r in run['records']:
        assert r['captions_per_image'] == 2 and r['images'] == 6
        assert (r['metrics']['kid']['n_real'], r['metrics']['kid']['n_fake']) == (6, 12)
        assert r['metrics']['r_precision']['n'] == 12
    r = run['records'][-1]
    assert r['metrics'] == offline(tracker, os.path.join(run['model_dir'], r['checkpoint']), fid=False)
    # an improving evaluation with no checkpoint of its own: netG_best.pth by torch.save, equal to save_model's file
    from sbagan.track import Best
    gan = algo.gan
    tracker.best = Best('kid.kid', run['model_dir'])
    rec = tracker.evaluate(gan.netG, None, 7, 99, None, None)
    assert rec['checkpoint'] is None and rec['metrics'] == r['metrics']         # (the weights of the final record)
    assert json.load(open(os.path.join(run['model_dir'], 'best.json')))['epoch'] == 7
    algo.save_model(gan.netG, gan.flatG.ema_params(), gan.netsD, 7)
    with open(os.path.join(run['model_dir'], 'netG_best.pth'), 'rb') as f:
        best = f.read()
    with open(os.path.join(run['model_dir'], 'netG_epoch_7.pth'), 'rb') as f:
        assert best == f.read()
    capsys.readouterr()


def test_bert_trainer_tracks(toy, det):
    """the BERT text side: trainer_bert._encode in prepare(), words_embs at the WORDS_NUM width, a record equal to its
    offline evaluation, training undisturbed"""
    import model_bert
    a, b = trained(toy, 'bert', track=1, max_epoch=1), trained(toy, 'bert', max_epoch=1)
    assert b['records'] is None and [r['epoch'] for r in a['records']] == [0, 1]
    assert sorted(a['files']) == sorted(b['files']) and 'netG_epoch_1.pth' in a['files']
    for name in a['files']:
        for k in a['files'][name]:
            assert torch.equal(a['files'][name][k], b['files'][name][k]), (name, k)
    for k in a['state']:
        assert torch.equal(a['state'][k], b['state'][k]), k
    assert same_generator_states(a['rng'], b['rng'])
    assert a['records'][0]['metrics'] == a['records'][1]['metrics']          # (the same weights twice)
    tracker = a['algo'].tracker
    assert type(tracker.dataset).__module__ == 'datasets_bert'
    assert tuple(tracker.words_embs.shape) == (5, 256, WORDS_NUM) and tuple(tracker.mask.shape) == (5, WORDS_NUM)
    r = a['records'][-1]
    assert r['metrics'] == offline(tracker, os.path.join(a['model_dir'], r['checkpoint']), fid=False,
                                   G_NET=model_bert.G_NET)


# ------------------------------------------------------------------ 5. the best weights
def test_best_names_the_argmin_and_holds_that_checkpoint(toy, det):
    run = trained(toy, 'replay', track=1, best='kid.kid')
    kids = [r['metrics']['kid']['kid'] for r in run['records']]
    k = int(np.argmin(kids))                                           # (the first of equal minima: ties keep the earlier)
    held = json.load(open(os.path.join(run['model_dir'], 'best.json')))
    r = run['records'][k]
    assert held == {'key': 'kid.kid', 'value': kids[k], 'epoch': r['epoch'], 'iteration': r['iteration']}
    with open(os.path.join(run['model_dir'], 'netG_best.pth'), 'rb') as f:
        best = f.read()
    with open(os.path.join(run['model_dir'], r['checkpoint']), 'rb') as f:
        assert best == f.read()


# ------------------------------------------------------------------ 6. the fused inference generator
def test_fused_inference_tracks_and_leaves_training_undisturbed(toy, det):
    a, b = trained(toy, 'replay', track=1, fused=True), trained(toy, 'replay')
    assert a['recorded']
    assert_undisturbed(a, b)
    for r in a['records']:
        assert np.isfinite(r['metrics']['kid']['kid']) and sorted(r['metrics']) == ['kid', 'prdc', 'r_precision']


# ------------------------------------------------------------------ 7. the entry points
class Stub(object):
    made = []

    def __init__(self, output_dir, dataloader, n_words, ixtoword, **kw):
        Stub.made.append(self)

    def train(self):
        pass

    def sampling(self, split_dir):
        pass


def _yml(tmp_path, root, flag):
    import yaml
    yml = tmp_path / ('toy_%d.yml' % flag)
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'toy', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0, 'B_VALIDATION': True,
        'TREE': {'BRANCH_NUM': 2, 'BASE_SIZE': 64}, 'GAN': {'GF_DIM': 32, 'DF_DIM': 64},
        'TRAIN': {'FLAG': bool(flag), 'NET_E': '', 'NET_G': '', 'BATCH_SIZE': B, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': WORDS_NUM}}))
    return str(yml)


FLAGS = ['--track', '2', '--track_split', 'test', '--track_n', '5', '--track_captions', '2', '--track_best', 'kid.kid',
         '--kid', '--prdc', '2']


def test_entry_points_hand_the_flags_over(toy, tmp_path, monkeypatch, capsys):
    import main
    import main_bert
    import trainer_bert
    from miscc.config import reset_cfg
    from test_bert_entry_gpu import _bert_dir
    (tmp_path / 'cwd').mkdir()
    monkeypatch.chdir(tmp_path / 'cwd')
    monkeypatch.setattr(trainer_bert, 'condGANTrainer', Stub)
    Stub.made = []
    on, off = _yml(tmp_path, toy['root'], 1), _yml(tmp_path, toy['root'], 0)
    bert = ['--bert_dir', _bert_dir(tmp_path)]

    def run(mod, argv):
        reset_cfg()
        capsys.readouterr()
        if mod is main:
            mod.main(argv, make_trainer=Stub)
        else:
            mod.main(argv + bert)
        return Stub.made[-1], capsys.readouterr().out

    for mod in (main, main_bert):
        algo, text = run(mod, ['--cfg', on, '--manualSeed', '5'] + FLAGS)
        assert (algo.track, algo.track_split, algo.track_n, algo.track_captions, algo.track_best) == \
            (2, 'test', 5, 2, 'kid.kid')
        assert algo.kid is True and algo.prdc == 2
        assert 'ignored outside training' not in text and 'not tracked' not in text
        algo, text = run(mod, ['--cfg', on, '--manualSeed', '5'])
        assert algo.track == 0 and '--track' not in text
        # outside training: one line, and the trainer keeps its defaults
        algo, text = run(mod, ['--cfg', off] + FLAGS)
        assert text.count('--track is ignored outside training') == 1
        assert getattr(algo, 'track', 0) == 0 and 'not tracked' not in text
        # the evaluators that stay out of training: one line naming them
        algo, text = run(mod, ['--cfg', on, '--manualSeed', '5', '--ms_ssim', '2', '--swd', '8', '--nearest', '1'] + FLAGS)
        assert text.count('--track: --ms_ssim, --swd, --nearest are not tracked in training (sampling only)') == 1
        assert text.count('not tracked') == 1 and algo.track == 2
        algo, text = run(mod, ['--cfg', on, '--manualSeed', '5', '--swd', '8'])
        assert 'not tracked' not in text                               # (without --track nothing is said)
    reset_cfg()


def test_the_trainer_refuses_what_only_the_configuration_can_tell(toy, det, tmp_path):
    from trainer import condGANTrainer
    ds = toy['ds']
    algo = condGANTrainer(str(tmp_path), [], ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.kid, algo.track, algo.track_captions = True, 1, 3              # TEXT.CAPTIONS_PER_IMAGE is 2
    with pytest.raises(ValueError, match='track_captions must be from 1 to TEXT.CAPTIONS_PER_IMAGE = 2'):
        algo._tracker()
    algo.track_captions, algo.kid = 1, False
    with pytest.raises(ValueError, match='track needs at least one of fid, kid, prdc, r_precision'):
        algo._tracker()
    algo.kid, algo.track = True, 0
    assert algo._tracker() is None
