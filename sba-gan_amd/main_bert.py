"""Entry point of the BERT path with the reference's command line (AttnGAN2/code/main_bert.py):

    python main_bert.py --cfg cfg/bird_style.yml --gpu 0 [--data_dir ...] [--bert_dir DIR] [--manualSeed N]
    python main_bert.py --cfg cfg/eval_bird.yml  ...      (sampling / the style-mixing examples)

main.py with datasets_bert.TextDataset and trainer_bert.condGANTrainer (BertEncoder text side, model_bert
generators).  --bert_dir: a local HuggingFace BERT directory (config, weights, vocab.txt)."""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import main as main_rnn  # noqa: E402
from datasets_bert import TextDataset  # noqa: E402
from main import build_example_dic  # noqa: E402,F401
from miscc import cli  # noqa: E402


def parse_args(argv=None):
    return cli.options('Train a AttnGAN network', 'cfg/bird_style.yml', argv, bert=True, gan=True)


def gen_example(wordtoix, algo):
    algo.gen_example(build_example_dic(wordtoix))


def main(argv=None):
    args = parse_args(argv)

    def dataset(*a, **kw):
        return TextDataset(*a, bert_dir=args.bert_dir, **kw)

    def make_trainer(output_dir, dataloader, n_words, ixtoword):
        from trainer_bert import condGANTrainer
        return condGANTrainer(output_dir, dataloader, n_words, ixtoword, bert_dir=args.bert_dir)

    main_rnn.main(args=args, dataset_cls=dataset, make_trainer=make_trainer)


if __name__ == '__main__':
    main()
