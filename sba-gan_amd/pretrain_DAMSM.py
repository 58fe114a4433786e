"""DAMSM pre-training with the reference's entry point (AttnGAN2/code/pretrain_DAMSM.py):

    python pretrain_DAMSM.py --cfg cfg/DAMSM/bird.yml --gpu 0 [--data_dir ...] [--manualSeed N]

train / evaluate / build_models keep the reference's signatures; the per-batch work is sbagan.damsm.DAMSMStep
(HIP kernels).  --attention_maps: the reference's Image/attention_maps<step>.png (sbagan.visualize.build_super_images)
wherever the interval log line is printed.  --device_data [--device_data_gb G]: both splits are decoded once into a
device-resident cache and every batch is cropped, flipped and normalised there (sbagan.device_data).  --replay (training
only): the update is ONE recording over a static batch slot (sbagan.damsm.DAMSMSlotStep), the losses are
read only where the interval line is printed.  --retrieval E: after the validation pass of every E-th epoch and of the
last one, the whole validation split is ranked both ways (sbagan.retrieval): one printed line and one JSON
line in Model/retrieval.jsonl.  --retrieval_only: the pair of TRAIN.NET_E is ranked once, retrieval.json is written and
nothing is trained.  --track E and its companions belong to GAN training (main.py): parsed here and ignored."""
import json
import os
import sys
import time

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from datasets import TextDataset, as_batch, prepare_data  # noqa: E402,F401
from miscc import cli, transforms  # noqa: E402
from miscc.config import cfg  # noqa: E402
from miscc.utils import mkdir_p  # noqa: E402
from model import CNN_ENCODER, RNN_ENCODER  # noqa: E402

UPDATE_INTERVAL = 50


def parse_args(argv=None):
    return cli.options('Train a DAMSM network', 'cfg/DAMSM/bird.yml', argv)


def train(dataloader, cnn_model, rnn_model, batch_size, labels, optimizer, epoch, ixtoword, image_dir,
          max_steps=None, attention_maps=False):
    """pretrain_DAMSM.py:49-130.  `optimizer` is the sbagan.damsm.DAMSMStep that owns the flat parameter buffers
    and the fused Adam (build it once per run, call .set_lr(lr) per epoch like the reference re-creates Adam)."""
    cnn_model.train()
    rnn_model.train()
    s0 = s1 = w0 = w1 = 0.0
    count = (epoch + 1) * len(dataloader)
    start_time = time.time()
    # --replay: `optimizer` is a sbagan.damsm.DAMSMSlotStep -- the batch goes into its slot (a bound device loader has put
    # it there already), the update is one re-issued recording, and the host reads the losses only where it prints them
    slot_step = optimizer if hasattr(optimizer, 'read_losses') else None
    for step, data in enumerate(dataloader, 0):
        if slot_step is not None:
            imgs, captions, cap_lens, class_ids, keys = slot_step.load(as_batch(data))
            slot_step.train()
        else:
            imgs, captions, cap_lens, class_ids, keys = as_batch(data)
            out = optimizer.step(imgs[-1], captions, cap_lens, class_ids)
            w0 += float(out['w_loss0']); w1 += float(out['w_loss1'])
            s0 += float(out['s_loss0']); s1 += float(out['s_loss1'])
        if step % UPDATE_INTERVAL == 0:
            count = epoch * len(dataloader) + step
            if slot_step is not None:       # means over the batches since the last line (the only host sync)
                m = slot_step.read_losses()
                means = m['s_loss0'], m['s_loss1'], m['w_loss0'], m['w_loss1']
            else:
                means = s0 / UPDATE_INTERVAL, s1 / UPDATE_INTERVAL, w0 / UPDATE_INTERVAL, w1 / UPDATE_INTERVAL
            elapsed = time.time() - start_time
            print('| epoch {:3d} | {:5d}/{:5d} batches | ms/batch {:5.2f} | s_loss {:5.2f} {:5.2f} | '
                  'w_loss {:5.2f} {:5.2f}'.format(epoch, step, len(dataloader), elapsed * 1000. / UPDATE_INTERVAL,
                                                  *means))
            s0 = s1 = w0 = w1 = 0.0
            if attention_maps:
                save_attention_maps(cnn_model, rnn_model, imgs[-1], captions, cap_lens, ixtoword,
                                    '%s/attention_maps%d.png' % (image_dir, step))
            start_time = time.time()
        if max_steps is not None and step + 1 >= max_steps:
            break
    return count


def save_attention_maps(cnn_model, rnn_model, imgs, captions, cap_lens, ixtoword, path):
    """pretrain_DAMSM.py:108-117: the word-to-region maps of (at most) the first 8 samples over their own images.  Both
    encoders run in eval mode without gradients (no dropout draw, no running-statistic update) and go back to theirs.
    Unlike the reference, which draws the maps of the training forward itself, this is a SECOND forward of the logged
    batch, after the optimizer step: the picture shows the updated weights, and every logged interval pays one more
    forward of 8 samples (the fused training step keeps no attention maps)."""
    from PIL import Image
    from sbagan.visualize import build_super_images, damsm_attention_maps
    n = min(8, imgs.size(0))
    modes = cnn_model.training, rnn_model.training
    cnn_model.eval()
    rnn_model.eval()
    try:
        with torch.no_grad():
            region_features, _ = cnn_model(imgs[:n])
            if hasattr(rnn_model, 'init_hidden'):
                words_emb, _ = rnn_model(captions[:n], cap_lens[:n], rnn_model.init_hidden(n))
            else:
                words_emb, _ = rnn_model(captions[:n])
    finally:
        cnn_model.train(modes[0])
        rnn_model.train(modes[1])
    maps = damsm_attention_maps(region_features, words_emb, cap_lens[:n], cfg.TRAIN.SMOOTH.GAMMA1)
    img_set, _ = build_super_images(imgs[:n], captions[:n], ixtoword, maps, region_features.size(2))
    Image.fromarray(img_set).save(path)


def evaluate(dataloader, cnn_model, rnn_model, batch_size, damsm=None):
    """pretrain_DAMSM.py:133-163: mean sentence / words loss over (at most) 50 validation batches."""
    cnn_model.eval()
    rnn_model.eval()
    s_total = w_total = 0.0
    step = 0
    for step, data in enumerate(dataloader, 0):
        real_imgs, captions, cap_lens, class_ids, keys = as_batch(data)
        s, w = damsm.evaluate(real_imgs[-1], captions, cap_lens, class_ids)
        s_total += float(s)
        w_total += float(w)
        if step == 50:
            break
    n = max(step, 1)
    return s_total / n, w_total / n


def retrieval(dataset_val, dataloader_val, cnn_model, rnn_model, imsize):
    """the retrieval figures of the encoder pair over the whole validation split, every caption of every image
    (sbagan.retrieval.Retrieval.result).  Images are centre-cropped, from the device cache when the validation loader has
    one; no global generator is consumed and both encoders go back to the mode they were in."""
    from sbagan.retrieval import evaluate_split
    return evaluate_split(dataset_val, cnn_model, rnn_model, cfg.TRAIN.BATCH_SIZE, imsize, int(imsize * 76 / 64),
                          cache=getattr(dataloader_val, 'cache', None), workers=cfg.WORKERS).result()


def build_models(n_words, batch_size):
    """pretrain_DAMSM.py:166-193."""
    text_encoder = RNN_ENCODER(n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)
    image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
    labels = torch.arange(batch_size, dtype=torch.int64)
    start_epoch = 0
    if cfg.TRAIN.NET_E != '':
        text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
        print('Load ', cfg.TRAIN.NET_E)
        name = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')     # (the pair is saved side by side)
        image_encoder.load_state_dict(torch.load(name, map_location='cpu'))
        print('Load ', name)
        start_epoch = cli.epoch_of(cfg.TRAIN.NET_E) + 1                     # text_encoder<epoch>.pth
        print('start_epoch', start_epoch)
    dev = torch.device('cuda', cfg.GPU_ID)
    return text_encoder.to(dev), image_encoder.to(dev), labels.to(dev), start_epoch


def main(argv=None, max_steps=None, args=None, dataset_cls=TextDataset, build=None, make_step=None):
    """`args` / `dataset_cls` / `build` (n_words, batch_size -> text encoder, image encoder, labels, start epoch): the
    BERT entry point (pretrain_DAMSM_bert.py) passes its own; the defaults are this script's.  `make_step`: with --replay,
    what builds the slot step (sbagan.damsm.DAMSMSlotStep's signature; the tests pass eager=True through it)."""
    args = parse_args(argv) if args is None else args
    build = build_models if build is None else build
    cli.configure(args)
    retrieval_only = bool(getattr(args, 'retrieval_only', False))
    if retrieval_only and cfg.TRAIN.NET_E == '':
        raise RuntimeError('--retrieval_only ranks a trained pair: set TRAIN.NET_E to its text_encoder<N>.pth')
    output_dir = cli.output_dir()
    model_dir, image_dir = os.path.join(output_dir, 'Model'), os.path.join(output_dir, 'Image')
    mkdir_p(model_dir)
    mkdir_p(image_dir)
    torch.cuda.set_device(cfg.GPU_ID)
    imsize = cli.image_size()
    batch_size = cfg.TRAIN.BATCH_SIZE
    image_transform = transforms.Compose([transforms.Scale(int(imsize * 76 / 64)), transforms.RandomCrop(imsize),
                                          transforms.RandomHorizontalFlip()])
    dataset = dataset_cls(cfg.DATA_DIR, 'train', base_size=cfg.TREE.BASE_SIZE, transform=image_transform)
    print(dataset.n_words, dataset.embeddings_num)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, drop_last=True, shuffle=True,
                                             num_workers=int(cfg.WORKERS))
    dataset_val = dataset_cls(cfg.DATA_DIR, 'test', base_size=cfg.TREE.BASE_SIZE, transform=image_transform)
    dataloader_val = torch.utils.data.DataLoader(dataset_val, batch_size=batch_size, drop_last=True, shuffle=True,
                                                 num_workers=int(cfg.WORKERS))
    if getattr(args, 'device_data', False):      # both splits cached on the device, batches made there
        from sbagan import device_data
        if not retrieval_only:
            dataloader = device_data.from_cfg(dataset, imsize, args.manualSeed, args.device_data_gb)
        dataloader_val = device_data.from_cfg(dataset_val, imsize, args.manualSeed + 1, args.device_data_gb)
    text_encoder, image_encoder, labels, start_epoch = build(dataset.n_words, batch_size)
    if retrieval_only:      # the loaded pair, ranked once: no training, no checkpoint
        result = retrieval(dataset_val, dataloader_val, image_encoder, text_encoder, imsize)
        from sbagan.retrieval import format_line
        print(format_line(start_epoch - 1, result))
        with open(os.path.join(output_dir, 'retrieval.json'), 'w') as f:
            json.dump(dict(result, net_e=cfg.TRAIN.NET_E), f, indent=1, sort_keys=True)
        return output_dir
    from sbagan.damsm import DAMSMSlotStep, DAMSMStep
    from sbagan.encoders import BertEncoder
    replay = bool(getattr(args, 'replay', False)) and cfg.TRAIN.FLAG
    if replay and isinstance(text_encoder, BertEncoder):
        print('--replay is ignored by DAMSM pre-training with the BERT text side (its dropout offset is a host argument)')
        replay = False
    if replay:      # the update as one recording over a static batch slot
        make_step = DAMSMSlotStep if make_step is None else make_step
        damsm = make_step(text_encoder, image_encoder, batch_size, imsize, lr=cfg.TRAIN.ENCODER_LR,
                          levels=cfg.TREE.BRANCH_NUM)
        if hasattr(dataloader, 'bind'):
            dataloader.bind(damsm.slot)     # the device loader writes every training batch straight into the slot
    else:
        damsm = DAMSMStep(text_encoder, image_encoder, batch_size, lr=cfg.TRAIN.ENCODER_LR)
    retrieval_every = int(getattr(args, 'retrieval', 0) or 0)
    try:
        lr = cfg.TRAIN.ENCODER_LR
        for epoch in range(start_epoch, cfg.TRAIN.MAX_EPOCH):
            damsm.set_lr(lr)
            train(dataloader, image_encoder, text_encoder, batch_size, labels, damsm, epoch, dataset.ixtoword,
                  image_dir, max_steps=max_steps, attention_maps=bool(getattr(args, 'attention_maps', False)))
            print('-' * 89)
            if len(dataloader_val) > 0:
                s_loss, w_loss = evaluate(dataloader_val, image_encoder, text_encoder, batch_size, damsm)
                print('| end epoch {:3d} | valid loss {:5.2f} {:5.2f} | lr {:.5f}|'.format(epoch, s_loss, w_loss, lr))
            last = epoch + 1 >= cfg.TRAIN.MAX_EPOCH or max_steps is not None
            if retrieval_every and len(dataset_val) > 0 and (epoch % retrieval_every == 0 or last):
                from sbagan.retrieval import format_line
                result = retrieval(dataset_val, dataloader_val, image_encoder, text_encoder, imsize)
                print(format_line(epoch, result))
                with open(os.path.join(model_dir, 'retrieval.jsonl'), 'a') as f:
                    f.write(json.dumps(dict(result, epoch=epoch, lr=lr), sort_keys=True) + '\n')
            print('-' * 89)
            if lr > cfg.TRAIN.ENCODER_LR / 10.:
                lr *= 0.98
            if epoch % cfg.TRAIN.SNAPSHOT_INTERVAL == 0 or epoch == cfg.TRAIN.MAX_EPOCH:
                torch.save(image_encoder.state_dict(), '%s/image_encoder%d.pth' % (model_dir, epoch))
                torch.save(text_encoder.state_dict(), '%s/text_encoder%d.pth' % (model_dir, epoch))
                print('Save G/Ds models.')
            if max_steps is not None:
                break
    except KeyboardInterrupt:
        print('-' * 89)
        print('Exiting from training early')
    finally:
        if getattr(dataloader, 'slot', None) is not None:
            dataloader.bind(None)
    return model_dir


if __name__ == '__main__':
    main()
