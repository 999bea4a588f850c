#!/usr/bin/env python
"""Evaluation script: scores a directory of held-out clips with a checkpoint
and prints one JSON line

    {"nll_per_sample": .., "bits_per_sample": .., "accuracy": .., "samples": .., "clips": ..}

(nats and bits per predicted sample, top-1 accuracy of the next-sample
prediction).  The clips are prepared as train.py's reader prepares them
(wavenet/evaluate.py's ValidationSet: sorted files, one pass, pieces per
file; with --lc_features mel, or a checkpoint that train.py --lc_features
wrote, the local conditioning is computed on the device from each batch's
audio and no <clip>.npy is read); the model flags are generate.py's, the
checkpoint is loaded as generate.py loads it (wavenet/checkpoint.py),
--use_ema true scores the checkpoint's EMA weights.  Without --sample_size
whole utterances are scored, batched by length.
"""
from __future__ import print_function

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

from wavenet import features, local_condition  # noqa: E402
from wavenet.checkpoint import (  # noqa: E402
    open_ema_checkpoint, restore, stored_lc_features)
from wavenet.cli import model_from_params, str_to_bool  # noqa: E402

BATCH_SIZE = 8
SILENCE_THRESHOLD = 0.3        # train.py's
WAVENET_PARAMS = './wavenet_params.json'   # generate.py's


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description='WaveNet evaluation script')
    p.add_argument('checkpoint', type=str,
                   help='Which model checkpoint to evaluate')
    p.add_argument('--data_dir', type=str, required=True,
                   help='The directory containing the held-out wav files.')
    p.add_argument('--use_ema', type=str_to_bool, default=False,
                   help='score the checkpoint\'s exponential moving average '
                   'of the weights (train.py --ema_decay)')
    p.add_argument('--sample_size', type=int, default=None,
                   help='Cut every file into pieces of this many samples '
                   '(default: whole utterances).')
    p.add_argument('--batch_size', type=int, default=BATCH_SIZE)
    p.add_argument('--max_batches', type=int, default=None,
                   help='Score at most this many batches (default: all).')
    p.add_argument('--silence_threshold', type=float,
                   default=SILENCE_THRESHOLD)
    p.add_argument('--wavenet_params', type=str,
                   default=WAVENET_PARAMS)
    p.add_argument('--gc_channels', type=int, default=None)
    p.add_argument('--gc_cardinality', type=int, default=None)
    p.add_argument('--lc_channels', type=int, default=None,
                   help='Local conditioning: channels of the features in '
                   '<clip>.npy next to every wav.')
    p.add_argument('--lc_hop', type=int, default=None,
                   help='audio samples per feature frame')
    p.add_argument('--lc_upsample_scales', type=str, default=None,
                   help='the scales of the model\'s learned upsampler '
                   '(train.py --lc_upsample_scales), e.g. 4,5,10')
    p.add_argument('--lc_context', type=int, default=None,
                   help='P of the model\'s frame-context convolution '
                   '(train.py --lc_context)')
    features.add_cli_flags(
        p, '  Default: the checkpoint\'s \'lc_features\' (train.py '
        '--lc_features), whose settings the other --lc_* flags default to; '
        '`none` reads <clip>.npy files whatever the checkpoint says.')
    return p.parse_args(argv)


def main(argv=None):
    args = get_arguments(argv)
    if args.gc_channels is not None and args.gc_cardinality is None:
        print('Globally conditioning but gc_cardinality not specified.')
        return 1
    if args.batch_size < 1:
        print('--batch_size must be positive')
        return 1
    with open(args.wavenet_params, 'r') as f:
        wavenet_params = json.load(f)
    try:
        stored = stored_lc_features(args.checkpoint)
        if args.lc_channels is None and args.lc_features != 'none' and \
                stored is not None:
            # (a checkpoint trained on its own front end names its mels)
            args.lc_channels = stored.get('n_mels')
        if args.lc_upsample_scales is not None and args.lc_channels is None:
            raise ValueError('--lc_upsample_scales needs --lc_channels')
        lc_scales, lc_hop, lc_ctx = local_condition.parse_cli(
            args.lc_upsample_scales, args.lc_hop, args.lc_context)
        spec = features.spec_from_cli(args, wavenet_params['sample_rate'],
                                      args.lc_channels, lc_hop, stored)
        if spec is not None:
            lc_hop = spec.hop
    except ValueError as e:
        print(str(e))
        return 1
    if args.lc_channels is not None and not lc_hop:
        print('--lc_channels needs --lc_hop (audio samples per feature '
              'frame)')
        return 1
    ckpt = None
    if args.use_ema:
        ckpt, why = open_ema_checkpoint(args.checkpoint)
        if why:
            print(why)
            return 1
    from wavenet import evaluate as ev
    gc_enabled = args.gc_channels is not None
    try:
        data = ev.ValidationSet(
            args.data_dir, wavenet_params['sample_rate'],
            sample_size=args.sample_size,
            silence_threshold=args.silence_threshold, gc_enabled=gc_enabled,
            gc_cardinality=args.gc_cardinality,
            lc_channels=None if spec is not None else args.lc_channels,
            lc_hop=lc_hop, lc_frames=lc_scales is not None)
    except ValueError as e:
        print(str(e))
        return 1
    net = model_from_params(
        wavenet_params, args.batch_size,
        global_condition_channels=args.gc_channels,
        global_condition_cardinality=args.gc_cardinality,
        local_condition_channels=args.lc_channels,
        local_condition_upsample_scales=lc_scales,
        local_condition_context=lc_ctx)
    why = restore(net, args.checkpoint, args.use_ema, ckpt,
                  check_lc=args.lc_channels is not None)
    if why:
        print(why)
        return 1
    batches = data.batches(args.batch_size)
    if spec is not None:
        batches = ev.with_features(net, spec, batches)
    result = ev.evaluate(net, batches, args.max_batches)
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
