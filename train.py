#!/usr/bin/env python
"""Training script: MI355X counterpart of the reference's train.py.

Same flags, defaults, logdir rules and progress line as the reference
(train.py:22-101 flags, :142-180 directory validation, :104-134 checkpoint
save / restore with the step parsed from the file name, :310-311
`step N - loss = x, (y sec/step)`), driving the HIP WaveNetModel.  New:
  * --synthetic : train on generated sine clips instead of --data_dir wavs;
  * data-parallel when launched by torchrun (one rank per GPU, RCCL);
  * --store_metadata dumps a kernel-level Chrome trace (torch.profiler) every
    50th step in place of TF's RunMetadata timeline.
Checkpoints are torch files `model.ckpt-<step>` holding {reference variable
name: tensor}; scalars go to <logdir>/events.jsonl (TensorBoard is TF-only).
"""
from __future__ import print_function

import argparse
import glob
import json
import os
import re
import sys
import time
from datetime import datetime

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import features, local_condition, tf_checkpoint  # noqa: E402

BATCH_SIZE = 1
DATA_DIRECTORY = './VCTK-Corpus'
LOGDIR_ROOT = './logdir'
CHECKPOINT_EVERY = 50
NUM_STEPS = int(1e5)
LEARNING_RATE = 1e-3
WAVENET_PARAMS = './wavenet_params.json'
STARTED_DATESTRING = "{0:%Y-%m-%dT%H-%M-%S}".format(datetime.now())
SAMPLE_SIZE = 100000
L2_REGULARIZATION_STRENGTH = 0
SILENCE_THRESHOLD = 0.3
EPSILON = 0.001
CORPUS_SEED = 0             # --device_corpus: every rank's index, every run
MOMENTUM = 0.9


def _str_to_bool(s):
    if s.lower() not in ('true', 'false'):
        raise ValueError('Argument needs to be a boolean, got {}'.format(s))
    return s.lower() == 'true'


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description='WaveNet example network')
    p.add_argument('--batch_size', type=int, default=BATCH_SIZE,
                   help='How many wav files to process at once (per GPU).')
    p.add_argument('--data_dir', type=str, default=None,
                   help='The directory containing the VCTK corpus '
                        '(default: {}).'.format(DATA_DIRECTORY))
    p.add_argument('--store_metadata', type=bool, default=False,
                   help='Store a kernel trace every 50 steps.')
    p.add_argument('--logdir', type=str, default=None,
                   help='Directory for logs / checkpoints; continues training '
                   'if it holds a model. Not with --logdir_root / '
                   '--restore_from.')
    p.add_argument('--logdir_root', type=str, default=None,
                   help='Root under which a dated logdir is created.')
    p.add_argument('--restore_from', type=str, default=None,
                   help='Directory to restore the model from (new logdir).')
    p.add_argument('--checkpoint_every', type=int, default=CHECKPOINT_EVERY)
    p.add_argument('--num_steps', type=int, default=NUM_STEPS)
    p.add_argument('--learning_rate', type=float, default=LEARNING_RATE)
    p.add_argument('--wavenet_params', type=str, default=WAVENET_PARAMS)
    p.add_argument('--sample_size', type=int, default=SAMPLE_SIZE,
                   help='Concatenate and cut audio samples to this many '
                   'samples.')
    p.add_argument('--l2_regularization_strength', type=float,
                   default=L2_REGULARIZATION_STRENGTH)
    p.add_argument('--silence_threshold', type=float,
                   default=SILENCE_THRESHOLD)
    p.add_argument('--optimizer', type=str, default='adam',
                   choices=['adam', 'sgd', 'rmsprop'])
    p.add_argument('--momentum', type=float, default=MOMENTUM)
    p.add_argument('--histograms', type=_str_to_bool, default=False)
    p.add_argument('--gc_channels', type=int, default=None,
                   help='Number of global condition channels.')
    p.add_argument('--dp_overlap_allreduce', type=_str_to_bool, default=False,
                   help='Data-parallel runs: all-reduce the skip / '
                        'post-processing gradients on a communication stream '
                        'beside the backward stack (two calls per step) '
                        'instead of one all-reduce at the update.  Off by '
                        'default: `bench.py --gpus N` times both schedules on '
                        'the node at hand -- switch it on where that run '
                        'reports allreduce_calls == 2 and overlap_failed false.')
    p.add_argument('--synthetic', action='store_true',
                   help='Train on synthetic sine clips (no --data_dir needed).')
    p.add_argument('--gc_cardinality', type=int, default=None,
                   help='Only with --synthetic: number of speaker ids.')
    p.add_argument('--lc_channels', type=int, default=None,
                   help='Local conditioning: channels of the per-sample '
                        'features, read from <clip>.npy [frames, channels] '
                        'next to every wav (random features with '
                        '--synthetic).  Feature row t conditions the '
                        'prediction of sample t + 1.')
    p.add_argument('--lc_hop', type=int, default=None,
                   help='Local conditioning: audio samples per feature frame '
                        '(frames are upsampled by repetition).  Default 1 '
                        'with --synthetic.')
    p.add_argument('--lc_upsample_scales', type=str, default=None,
                   help='Local conditioning: upsample the frames on the device '
                        'with a learned network of transposed convolutions, '
                        'one layer per scale, e.g. 4,5,10 (hop = their '
                        'product; --lc_hop must be absent or equal to it).')
    p.add_argument('--lc_context', type=int, default=None,
                   help='Local conditioning: a learned convolution over 2P + 1 '
                        'frames (P frames either side, channels to channels) '
                        'in front of the upsampler, 0 <= P <= 8.  Needs '
                        '--lc_upsample_scales.')
    p.add_argument('--mask_padding', type=_str_to_bool, default=False,
                   help='Batches of clips of different lengths: pass the '
                        'clips\' real lengths to the loss, so that the zero '
                        'padding behind the shorter ones is neither learned '
                        'nor counted in the mean (WaveNetModel.loss, '
                        '`lengths`).  Prints the real samples per step beside '
                        'the loss.')
    p.add_argument('--clip_norm', type=float, default=None,
                   help='Clip the gradient by its global norm '
                        '(tf.clip_by_global_norm) inside the update: the norm '
                        'of the whole averaged gradient, L2 term included, '
                        'scaled down to this value when it is larger.  The '
                        'norm before clipping is logged beside the loss.  '
                        'Default: no clipping.')
    p.add_argument('--ema_decay', type=float, default=None,
                   help='Keep an exponential moving average of the weights '
                        'with this decay, in [0, 1) (e.g. 0.9999); saved as '
                        '`ema_variables` for generate.py --use_ema true.  '
                        'Default: none.')
    p.add_argument('--validation_dir', type=str, default=None,
                   help='Directory of held-out wav files (and <clip>.npy '
                        'features with --lc_channels): scored with '
                        'WaveNetModel.score every --validate_every steps and '
                        'after the last step; every rank scores its shard of '
                        'the files.  Default: no validation.')
    p.add_argument('--validate_every', type=int, default=None,
                   help='Validate after every step divisible by this '
                        '(default: --checkpoint_every).')
    p.add_argument('--validation_batches', type=int, default=None,
                   help='Score at most this many batches per rank and '
                        'validation (default: the whole directory).')
    p.add_argument('--validate_ema', type=_str_to_bool, default=False,
                   help='Validate the exponential moving average of the '
                        'weights instead of the weights (needs --ema_decay).')
    features.add_cli_flags(
        p, '  Needs --lc_channels and --lc_hop or --lc_upsample_scales; '
        'with --mask_padding true the clips\' lengths go to the front end '
        'too.  The settings are stored in every checkpoint (\'lc_features\') '
        'and --validation_dir is scored through the same front end.')
    p.add_argument('--device_corpus', type=_str_to_bool, default=False,
                   help='Keep the whole trimmed --data_dir on the device and '
                        'cut every training batch there with a kernel '
                        '(wavenet/corpus.py): no reader thread, no copy per '
                        'step.  The order is a pure function of the step, so '
                        'a resumed run continues the same sequence.  Needs '
                        '--data_dir; not with --synthetic, nor with '
                        '--lc_channels read from <clip>.npy files (use '
                        '--lc_features mel).  Validation is unchanged.')
    p.add_argument('--crop', choices=['pieces', 'random'], default=None,
                   help='--device_corpus: pieces (default) cuts every '
                        'utterance into --sample_size pieces like the '
                        'reader; random draws one window of --sample_size '
                        'samples per utterance afresh every epoch.')
    p.add_argument('--lc_feature_context', choices=['piece', 'utterance'],
                   default=None,
                   help='--lc_features mel: piece (default) computes the '
                        'features of each batch as cut, a piece\'s edges see '
                        'zeros; utterance (needs --device_corpus true) '
                        'computes every utterance\'s frames once at load and '
                        'gives each piece the frames of its place in the '
                        'utterance.')
    args = p.parse_args(argv)
    # (--data_dir's default is filled in here, so that "not given" shows)
    data_dir_given = args.data_dir is not None
    if not data_dir_given:
        args.data_dir = DATA_DIRECTORY
    if args.device_corpus:
        if not data_dir_given:
            p.error('--device_corpus true needs --data_dir')
        if args.synthetic:
            p.error('--device_corpus true does not go with --synthetic')
        if args.lc_channels is not None and args.lc_features != 'mel':
            p.error('--device_corpus true reads no <clip>.npy features: '
                    '--lc_channels needs --lc_features mel with it')
        if args.crop == 'random' and not args.sample_size:
            p.error('--crop random needs --sample_size')
    elif args.crop is not None:
        p.error('--crop needs --device_corpus true')
    if args.lc_feature_context == 'utterance' and not (
            args.device_corpus and args.lc_features == 'mel'):
        p.error('--lc_feature_context utterance needs --device_corpus true '
                'and --lc_features mel')
    if args.lc_feature_context is not None and args.lc_features != 'mel':
        p.error('--lc_feature_context needs --lc_features mel')
    if args.lc_features == 'mel':
        if args.lc_channels is None:
            p.error('--lc_features mel needs --lc_channels (the number of '
                    'mels)')
        if args.lc_hop is None and args.lc_upsample_scales is None:
            p.error('--lc_features mel needs --lc_hop or '
                    '--lc_upsample_scales (hop = their product)')
        try:
            features.normalize_flags(args, corpus=args.device_corpus)
        except ValueError as e:
            p.error(str(e))
    elif features.cli_flags_given(args):
        p.error('%s needs --lc_features mel'
                % features.cli_flags_given(args)[0])
    return args


def validation_flags(args):
    """ValueError where the validation flags do not fit together."""
    if args.validate_ema and args.ema_decay is None:
        raise ValueError('--validate_ema true needs --ema_decay')
    if args.validation_dir is None:
        for flag in ('validate_every', 'validation_batches'):
            if getattr(args, flag) is not None:
                raise ValueError('--%s needs --validation_dir' % flag)
        if args.validate_ema:
            raise ValueError('--validate_ema needs --validation_dir')
    for flag in ('validate_every', 'validation_batches'):
        v = getattr(args, flag)
        if v is not None and v < 1:
            raise ValueError('--%s must be positive, got %d' % (flag, v))


def lc_upsample_scales(args):
    """(scales tuple, hop) of --lc_upsample_scales, or (None, args.lc_hop);
    ValueError for a malformed list or an --lc_hop that disagrees."""
    if args.lc_upsample_scales is not None and args.lc_channels is None:
        raise ValueError('--lc_upsample_scales needs --lc_channels')
    return local_condition.parse_cli(args.lc_upsample_scales, args.lc_hop,
                                     None)[:2]


def lc_context(args):
    """P of --lc_context (None without it); ValueError without
    --lc_upsample_scales or out of range."""
    if args.lc_context is None:
        return None
    return local_condition.parse_cli(args.lc_upsample_scales, None,
                                     args.lc_context)[2]


def checkpoint_path(logdir, step):
    return os.path.join(logdir, 'model.ckpt-{}'.format(step))


def save(net, logdir, step, optimizer=None, lc_features=None,
         device_corpus=None):
    """`optimizer`: its step count, slots and shadow go in as 'optimizer'
    and, with EMA weights, the shadow as 'ema_variables' (the keys of
    'variables').  `lc_features`: the front end's settings
    (features.checkpoint_entry), stored under 'lc_features'.
    `device_corpus`: the settings of --device_corpus (crop, seed,
    sample_size, lc_feature_context) and the index of the last batch taken
    ('batch'), stored under 'device_corpus'."""
    print('Storing checkpoint to {} ...'.format(logdir), end="")
    sys.stdout.flush()
    os.makedirs(logdir, exist_ok=True)
    path = checkpoint_path(logdir, step)
    ckpt = {'variables': net.state_dict(), 'step': step}
    if lc_features is not None:
        ckpt['lc_features'] = lc_features
    if device_corpus is not None:
        ckpt['device_corpus'] = device_corpus
    if optimizer is not None:
        ckpt['optimizer'] = optimizer.state_dict()
        if optimizer.ema_decay is not None:
            ckpt['ema_variables'] = optimizer.ema_state_dict(net)
    torch.save(ckpt, path)
    with open(os.path.join(logdir, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "{}"\n'.format(os.path.basename(path)))
    print(' Done.')


def latest_checkpoint(logdir):
    """Newest `model.ckpt-<step>` in logdir, or None."""
    marker = os.path.join(logdir, 'checkpoint')
    if os.path.exists(marker):
        name = open(marker).read().split('"')[1]
        path = os.path.join(logdir, name)
        # (a TensorFlow V2 checkpoint is a prefix: model.ckpt-N.index / .data-*)
        if os.path.exists(path) or tf_checkpoint.checkpoint_format(path):
            return path
    # only `model.ckpt-<step>` itself or a V2 prefix's `.index`: a V2 data
    # shard (`model.ckpt-N.data-00000-of-00001`) and `.meta` also end in
    # digits / start with the prefix, and must not be taken for a checkpoint
    found = {}
    for f in glob.glob(os.path.join(logdir, 'model.ckpt-*')):
        base = f[:-len('.index')] if f.endswith('.index') else f
        m = re.match(r'model\.ckpt-(\d+)$', os.path.basename(base))
        if m:
            found[base] = int(m.group(1))
    return max(found, key=found.get) if found else None


def load(net, logdir, optimizer=None, entries=None):
    """`optimizer`: restored from the checkpoint's 'optimizer' entry when it
    has one (checkpoints written before it existed, and the reference's own,
    have none: the optimizer then starts afresh, as it always did).
    `entries`: a dict that receives the checkpoint's 'device_corpus' entry."""
    print("Trying to restore saved checkpoints from {} ...".format(logdir),
          end="")
    path = latest_checkpoint(logdir) if os.path.isdir(logdir) else None
    if path is None:
        print(" No checkpoint found.")
        return None
    print("  Checkpoint found: {}".format(path))
    global_step = int(path.split('/')[-1].split('-')[-1])
    print("  Global step was: {}".format(global_step))
    print("  Restoring...", end="")
    if tf_checkpoint.checkpoint_format(path):
        # written by the reference's tf.train.Saver (train.py:104-114 there)
        tf_checkpoint.load_into(net, path)
    else:
        ckpt = torch.load(path, map_location='cpu')
        net.load_state_dict(ckpt['variables'])
        if optimizer is not None and 'optimizer' in ckpt:
            optimizer.load_state_dict(ckpt['optimizer'], net)
        if entries is not None and 'device_corpus' in ckpt:
            entries['device_corpus'] = ckpt['device_corpus']
    print(" Done.")
    return global_step


def stored_normalizer(logdir):
    """The normaliser entry in the 'lc_features' of logdir's newest
    checkpoint, or None (no checkpoint, not one of ours, no normaliser)."""
    path = latest_checkpoint(logdir) if os.path.isdir(logdir) else None
    if path is None or tf_checkpoint.checkpoint_format(path):
        return None
    entry = torch.load(path, map_location='cpu').get('lc_features') or {}
    return entry.get('normalizer')


def corpus_first_batch(stored, entry):
    """--device_corpus: step k of a run takes batch base + k.  A run continued
    in its logdir continues its step count (base 0).  A new training restored
    from a checkpoint starts at step 0: it goes on with the batch after the
    last one of the checkpoint's 'device_corpus' entry `stored` where that
    has this run's settings `entry`, else it starts the sequence again."""
    if stored is None:
        return 0
    if {k: stored.get(k) for k in entry} != entry:
        print("  The checkpoint's corpus settings {} differ: the corpus "
              "starts again.".format(stored))
        return 0
    base = int(stored.get('batch', -1)) + 1
    print('  Corpus batches continue at {}.'.format(base))
    return base


def get_default_logdir(logdir_root):
    return os.path.join(logdir_root, 'train', STARTED_DATESTRING)


def validate_directories(args):
    """Validate and arrange directory related arguments (train.py:142-180)."""
    if args.logdir and args.logdir_root:
        raise ValueError("--logdir and --logdir_root cannot be "
                         "specified at the same time.")
    if args.logdir and args.restore_from:
        raise ValueError(
            "--logdir and --restore_from cannot be specified at the same "
            "time. This is to keep your previous model from unexpected "
            "overwrites.\nUse --logdir_root to specify the root of the "
            "directory which will be automatically created with current date "
            "and time, or use only --logdir to just continue the training "
            "from the last checkpoint.")
    logdir_root = args.logdir_root or LOGDIR_ROOT
    logdir = args.logdir
    if logdir is None:
        logdir = get_default_logdir(logdir_root)
        print('Using default logdir: {}'.format(logdir))
    restore_from = args.restore_from or logdir
    return {'logdir': logdir, 'logdir_root': args.logdir_root,
            'restore_from': restore_from}


class SyntheticReader(object):
    """Sine-plus-noise clips of `sample_size` samples (BASELINE.md data)."""

    def __init__(self, sample_size, gc_cardinality=None, rank=0, seed=1234,
                 lc_channels=None, lc_hop=1):
        self.T, self.card = sample_size, gc_cardinality
        self.rng = np.random.default_rng(seed + rank)
        self.gc_category_cardinality = gc_cardinality
        self.count = rank * 1000003
        self.lc_channels, self.lc_hop = lc_channels, lc_hop

    def _clip(self):
        self.count += 1
        f = 110.0 * 2 ** ((self.count % 36) / 12.0)
        t = np.arange(self.T)
        x = 0.5 * np.sin(2 * np.pi * f * t / 16000.0) + \
            0.05 * self.rng.standard_normal(self.T)
        return np.clip(x, -1, 1).astype(np.float32), self.count

    def dequeue(self, n):
        clips = [self._clip() for _ in range(n)]
        self._last_ids = [c[1] for c in clips]
        return torch.from_numpy(np.stack([c[0] for c in clips]))[..., None]

    def dequeue_gc(self, n):
        return torch.tensor([(37 * i) % self.card for i in self._last_ids],
                            dtype=torch.int32)

    def dequeue_lc_frames(self, n):
        """Random frame-rate features [n, F, Lc] and offsets [n] in
        [0, 4 * lc_hop): sample t of clip i sits at position offsets[i] + t."""
        hop = self.lc_hop
        offs = self.rng.integers(0, 4 * hop, n)
        frames = (int(offs.max()) + self.T - 1) // hop + 1
        return (torch.from_numpy(self.rng.standard_normal(
            (n, frames, self.lc_channels)).astype(np.float32)),
            torch.from_numpy(offs.astype(np.int64)))

    def dequeue_lc(self, n):
        """Random frame-rate features upsampled by repetition: [n, T, Lc]."""
        from wavenet.audio_reader import upsample_lc
        frames = (self.T + self.lc_hop - 1) // self.lc_hop
        return torch.from_numpy(np.stack([
            upsample_lc(self.rng.standard_normal(
                (frames, self.lc_channels)).astype(np.float32),
                self.lc_hop, self.T) for _ in range(n)]))

    def dequeue_lengths(self, n):
        return torch.full((n,), self.T, dtype=torch.int64)

    def start_threads(self, *a, **k):
        return []


def main(argv=None):
    args = get_arguments(argv)
    try:
        lc_scales, lc_hop = lc_upsample_scales(args)
        lc_ctx = lc_context(args)
        validation_flags(args)
    except ValueError as e:
        print(str(e))
        return 1
    try:
        directories = validate_directories(args)
    except ValueError as e:
        print("Some arguments are wrong:")
        print(str(e))
        return 1
    logdir = directories['logdir']
    restore_from = directories['restore_from']
    # a restored model written somewhere else counts as a new training
    is_overwritten_training = logdir != restore_from

    from wavenet import WaveNetModel, AudioReader, optimizer_factory, parallel
    from wavenet.audio_reader import Coordinator
    rank, world, local = parallel.init_from_env(host_control_plane=True)
    if torch.cuda.is_available():
        torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))

    with open(args.wavenet_params, 'r') as f:
        wavenet_params = json.load(f)

    coord = Coordinator()
    # The reference computes `silence_threshold = None if below EPSILON` and
    # then passes the RAW flag to the reader (train.py:211-220; SURVEY Appendix
    # A: "do not fix silently") -- same here: `--silence_threshold 0` trims with
    # a threshold of 0 (only exactly silent frames go) instead of skipping the
    # trimming.
    silence_threshold = args.silence_threshold
    gc_enabled = args.gc_channels is not None
    lc_enabled = args.lc_channels is not None
    # --lc_features: the readers yield audio only, the features of every
    # batch are computed on the device from the batch itself
    spec = None
    try:
        spec = features.spec_from_cli(args, wavenet_params['sample_rate'],
                                      args.lc_channels, lc_hop,
                                      corpus=args.device_corpus)
    except (ValueError, OSError) as e:
        print(str(e))
        return 1
    # --lc_normalize corpus without --lc_stats: the corpus supplies the
    # statistics below.  A run continued in its logdir keeps the normaliser
    # of its checkpoint instead (--lc_normalize none / range still decide).
    lc_stats = features.FeatureStats.load(args.lc_stats) \
        if spec is not None and args.lc_stats is not None else None
    kept_norm = None
    if spec is not None and not is_overwritten_training and \
            args.lc_normalize in (None, 'corpus'):
        kept = stored_normalizer(restore_from)
        if kept is not None:
            kept_norm = features.Normalizer.from_entry(kept)
            print('  The checkpoint\'s feature normaliser continues.')
            spec = spec.with_normalizer(kept_norm)
    from_corpus = spec is not None and args.lc_normalize == 'corpus' and \
        args.lc_stats is None
    stats_sum = None
    if from_corpus and world > 1:
        def stats_sum(v):
            return parallel.sum_float64_over_ranks(
                v, 'cuda' if torch.cuda.is_available() else 'cpu')
    file_lc = None if spec is not None else args.lc_channels
    corpus = corpus_entry = corpus_lc = None
    if args.device_corpus:
        # the corpus on the device replaces the reader and its threads for
        # the training batches (wavenet/corpus.py)
        from wavenet.corpus import DeviceCorpus
        utt_ctx = args.lc_feature_context == 'utterance'
        corpus_norm = {}
        if utt_ctx and from_corpus:
            # the resident frames: summed and normalised in place at load
            corpus_norm = dict(normalize=kept_norm, stats_allreduce=stats_sum) \
                if kept_norm is not None else \
                dict(normalize='corpus', normalize_clip=args.lc_norm_clip,
                     stats_allreduce=stats_sum)
        try:
            corpus = reader = DeviceCorpus(
                args.data_dir, wavenet_params['sample_rate'], gc_enabled,
                sample_size=args.sample_size or None,
                silence_threshold=silence_threshold,
                crop=args.crop or 'pieces', seed=CORPUS_SEED, rank=rank,
                world=world, spec=spec if utt_ctx else None, **corpus_norm)
        except (ValueError, MemoryError) as e:
            print(str(e))
            return 1
        if from_corpus:
            if utt_ctx:
                lc_stats, spec = corpus.feature_stats, corpus.spec
            elif kept_norm is None:
                # no frames are resident: one pass over the utterances
                lc_stats = corpus.compute_feature_stats(spec, stats_sum)
            if kept_norm is None:
                spec = spec.with_normalizer(features.Normalizer.from_stats(
                    lc_stats, args.lc_norm_clip))
            elif lc_stats is not None:
                fresh = features.Normalizer.from_stats(lc_stats)
                if not (np.array_equal(fresh.shift, kept_norm.shift) and
                        np.array_equal(fresh.scale, kept_norm.scale)):
                    print('  The corpus\'s feature statistics differ from '
                          'the checkpoint\'s normaliser, which is kept.')
        if utt_ctx:
            corpus_lc = 'frames' if lc_scales is not None else 'rows'
        corpus_entry = dict(crop=args.crop or 'pieces', seed=CORPUS_SEED,
                            sample_size=args.sample_size or None,
                            lc_feature_context=args.lc_feature_context
                            or 'piece')
    elif args.synthetic:
        reader = SyntheticReader(args.sample_size,
                                 args.gc_cardinality if gc_enabled else None,
                                 rank=rank, lc_channels=file_lc,
                                 lc_hop=lc_hop or 1)
    else:
        if lc_enabled and not lc_hop:
            print('--lc_channels needs --lc_hop (audio samples per feature '
                  'frame)')
            return 1
        reader = AudioReader(args.data_dir, coord,
                             sample_rate=wavenet_params['sample_rate'],
                             gc_enabled=gc_enabled,
                             sample_size=args.sample_size,
                             silence_threshold=silence_threshold,
                             rank=rank, world=world, seed=rank,
                             lc_channels=file_lc,
                             lc_hop=lc_hop, lc_frames=lc_scales is not None)

    lc_entry = None if spec is None else features.checkpoint_entry(spec)
    if lc_stats is not None and rank == 0:
        os.makedirs(logdir, exist_ok=True)
        lc_stats.save(os.path.join(logdir, 'lc_stats.npz'))

    net = WaveNetModel(
        batch_size=args.batch_size,
        dilations=wavenet_params["dilations"],
        filter_width=wavenet_params["filter_width"],
        residual_channels=wavenet_params["residual_channels"],
        dilation_channels=wavenet_params["dilation_channels"],
        skip_channels=wavenet_params["skip_channels"],
        quantization_channels=wavenet_params["quantization_channels"],
        use_biases=wavenet_params["use_biases"],
        scalar_input=wavenet_params["scalar_input"],
        initial_filter_width=wavenet_params["initial_filter_width"],
        histograms=args.histograms,
        global_condition_channels=args.gc_channels,
        global_condition_cardinality=reader.gc_category_cardinality,
        residual_postproc=wavenet_params.get("residual_postproc", False),
        local_condition_channels=args.lc_channels,
        local_condition_upsample_scales=lc_scales,
        local_condition_context=lc_ctx)
    l2 = args.l2_regularization_strength or None
    try:
        optimizer = optimizer_factory[args.optimizer](
            learning_rate=args.learning_rate, momentum=args.momentum,
            clip_norm=args.clip_norm, ema_decay=args.ema_decay)
    except ValueError as e:
        print(str(e))
        return 1

    try:
        restored = {}
        saved_global_step = load(net, restore_from, optimizer, restored)
        if is_overwritten_training or saved_global_step is None:
            # the first training step will be saved_global_step + 1
            saved_global_step = -1
        corpus_base = 0
        if corpus is not None and is_overwritten_training:
            corpus_base = corpus_first_batch(restored.get('device_corpus'),
                                             corpus_entry)
    except Exception:
        print("Something went wrong while restoring checkpoint. "
              "We will terminate training to avoid accidentally overwriting "
              "the previous model.")
        raise
    parallel.broadcast_parameters(net)
    # every loss() below is followed by optimizer.minimize(): the skip /
    # post-processing gradients' all-reduce MAY start inside the backward pass
    # (opt-in: the schedule has not been measured on an N-GPU RCCL node yet)
    net.dp_overlap_allreduce = bool(args.dp_overlap_allreduce) and world > 1

    vset = None
    if args.validation_dir is not None:
        from wavenet import evaluate as ev
        # one deterministic pass per validation, this rank's shard of the
        # sorted files, prepared like the training pieces
        vset = ev.ValidationSet(
            args.validation_dir, wavenet_params['sample_rate'],
            sample_size=args.sample_size,
            silence_threshold=silence_threshold, gc_enabled=gc_enabled,
            gc_cardinality=reader.gc_category_cardinality,
            lc_channels=file_lc, lc_hop=lc_hop,
            lc_frames=lc_scales is not None, rank=rank, world=world)
    validate_every = args.validate_every or args.checkpoint_every

    threads = [] if corpus is not None else reader.start_threads()

    def corpus_at(k):
        """The 'device_corpus' entry of a checkpoint after step k."""
        return None if corpus is None else \
            dict(corpus_entry, batch=corpus_base + k)
    events = None
    if rank == 0:
        os.makedirs(logdir, exist_ok=True)
        events = open(os.path.join(logdir, 'events.jsonl'), 'a')

    step = None
    last_saved_step = saved_global_step
    pending = None            # (step, mean loss tensor, start time) not yet printed
    last_report = [None]
    last_run = validated = None   # --validation_dir: last step run / validated

    def report(k, mean_loss, started, real=None, norm=None):
        """Fetch step k's loss (waits for that step), check it, print / log the
        reference's line (train.py:310-311).  sec/step: from the previous line
        (the pipeline's cadence), or from the step's start for the first."""
        # (float(tensor) would wait for EVERYTHING queued on the stream, the
        # next step included: the loss went to a pinned scalar behind an event)
        host_scalar, done = mean_loss
        done.synchronize()
        loss_value = float(host_scalar)
        # (--clip_norm: the norm before clipping, copied behind the loss on
        # the same stream: complete once the loss's event is)
        norm_value = None if norm is None else float(norm[0])
        if not np.isfinite(loss_value):
            # every rank sees the same NaN mean: decide TOGETHER whether a
            # kernel reported an error, so that no rank is left waiting in
            # the next step's collectives
            dev_err = None
            try:
                net.check_device_errors()
            except Exception as e:
                dev_err = e
            if parallel.any_rank(dev_err is not None, net.device):
                raise dev_err or RuntimeError(
                    'rank %d: another rank reported an expired dependency '
                    'wait in a persistent stack launch at step %d'
                    % (rank, k))
        now = time.time()
        duration = now - (last_report[0] if last_report[0] is not None and
                          last_report[0] > started else started)
        last_report[0] = now
        if rank == 0:
            # (--mask_padding: `real` = the step's real samples, all ranks')
            print('step {:d} - loss = {:.3f}, ({:.3f} sec/step)'
                  .format(k, loss_value, duration) +
                  ('' if real is None else ', {:d} real samples'.format(real))
                  + ('' if norm_value is None else
                     ', grad norm = {:.3f}'.format(norm_value)))
            line = {'step': k, 'loss': loss_value, 'sec_per_step': duration}
            if norm_value is not None:
                line['grad_norm'] = norm_value
            if real is not None:
                line['real_samples'] = real
            events.write(json.dumps(line) + '\n')
            events.flush()

    def validate(k):
        """Score the validation set with the weights after step k's update
        (the EMA shadow with --validate_ema): every rank its shard, ONE sum
        over the ranks whatever a shard holds, rank 0 prints and logs."""
        import contextlib
        swap = ev.parameters_swapped(net, optimizer.ema_flat(net)) \
            if args.validate_ema else contextlib.nullcontext()
        with swap:
            batches = vset.batches(args.batch_size)
            if spec is not None:
                batches = ev.with_features(net, spec, batches)
            tot = ev.totals(net, batches, args.validation_batches)
        res = ev.summary(ev.sum_over_ranks(tot, net.device))
        if rank == 0:
            print('step {:d} - validation loss = {:.3f}, bits/sample = {:.3f}'
                  ', accuracy = {:.3f}'.format(
                      k, res['nll_per_sample'], res['bits_per_sample'],
                      res['accuracy']))
            events.write(json.dumps({
                'step': k, 'validation_loss': res['nll_per_sample'],
                'validation_bits': res['bits_per_sample'],
                'validation_accuracy': res['accuracy'],
                'validation_samples': res['samples']}) + '\n')
            events.flush()

    fetch_slots = {}

    def fetch_later(t, k, tag=0):
        """(pinned host scalar, event): the scalar holds t once the event has
        completed; two slots per `tag` used alternately (a slot is read before
        the step after next overwrites it)."""
        k = 2 * tag + (k & 1)
        if not t.is_cuda:
            class _Done(object):
                def synchronize(self):
                    pass
            return t.detach().reshape(()).clone(), _Done()
        if k not in fetch_slots:
            fetch_slots[k] = (torch.empty((), dtype=torch.float32).pin_memory(),
                              torch.cuda.Event())
        host_scalar, ev = fetch_slots[k]
        host_scalar.copy_(t.detach().reshape(()).float(), non_blocking=True)
        ev.record()
        return host_scalar, ev

    copy_stream = [None]

    def stage_in(host, k):
        """host [B, n] float tensor -> device tensor, copied on a stream of its
        own: the (pageable, hence host-blocking) copy then does not queue
        behind the previous step's kernels, and the training stream only
        waits for the copy.  (Pinned staging buffers measured 33 instead of
        9.6 ms per step on this platform, tools/h2d_probe.py.)"""
        if copy_stream[0] is None:
            copy_stream[0] = torch.cuda.Stream(device=net.device)
        with torch.cuda.stream(copy_stream[0]):
            dev = host.contiguous().to(net.device)
        torch.cuda.current_stream().wait_stream(copy_stream[0])
        dev.record_stream(torch.cuda.current_stream())
        return dev

    try:
        for step in range(saved_global_step + 1, args.num_steps):
            start_time = time.time()
            # every rank takes the same decision for this step (skip / common
            # clip length / abort) BEFORE any collective of the step is issued
            err = cplan = None
            lc, lc_off = None, 0
            try:
                if corpus is not None:
                    # the host index alone: T, lengths and speaker ids; the
                    # batch itself is cut on the device, below
                    cplan = corpus.plan(corpus_base + step, args.batch_size)
                    audio = None
                    lengths = cplan.n if args.mask_padding else None
                    gc = torch.from_numpy(cplan.gc) if gc_enabled else None
                else:
                    audio = reader.dequeue(args.batch_size)
                    lengths = \
                        reader.dequeue_lengths(args.batch_size).numpy() \
                        if args.mask_padding else None
                    gc = reader.dequeue_gc(args.batch_size) \
                        if gc_enabled else None
                    if spec is not None:
                        pass              # (from the staged batch, below)
                    elif lc_scales is not None:
                        # frames + offsets: the model upsamples on the device
                        lc, lc_off = reader.dequeue_lc_frames(args.batch_size)
                    elif lc_enabled:
                        lc = reader.dequeue_lc(args.batch_size)
            except Exception as e:        # e.g. a reader-thread failure
                err, audio, gc, lc, lengths = e, None, None, None, None
            n_t, all_ok = parallel.agree_step(
                0 if err is not None else
                cplan.T if cplan is not None else audio.shape[1],
                err is None, net.device)
            if not all_ok:
                raise RuntimeError('rank %d: a rank failed to produce a batch '
                                   'at step %d%s' % (rank, step, '' if err is
                                                     None else ': %r' % err))
            den = real = None
            if lengths is not None:
                # (cut to the common T like the rows; every rank's longest
                # real clip is then n_t samples, so the guard below looks at
                # the longest real length and decides the same on every rank)
                lengths = np.minimum(lengths, n_t)
                den = parallel.masked_denominator(lengths, net.device)
                real = int(round(den * world))
            if (n_t if lengths is None else int(lengths.max())) < 2:
                continue
            if corpus is not None:
                # (one or two launches on the training stream; no copy)
                cb = corpus.batch(corpus_base + step, args.batch_size, T=n_t,
                                  lc=corpus_lc)
                audio = cb.audio
                if corpus_lc == 'frames':
                    lc, lc_off = cb.frames, cb.offsets
                elif corpus_lc == 'rows':
                    lc = cb.rows
            else:
                audio = audio[:, :n_t]
            if lc is not None and lc_scales is None:
                lc = lc[:, :n_t]
            if audio.device.type == 'cpu' and net.device.type == 'cuda':
                # pinned staging + asynchronous copy: a pageable host tensor
                # handed to net.loss is copied synchronously BEHIND the previous
                # step's kernels, i.e. the host would wait for the device every
                # step and prepare the next batch while it idles
                audio = stage_in(audio.reshape(audio.shape[0], -1), step)
            if spec is not None and corpus_lc is None:
                # frames (offset 0) for an upsampler model, else rows
                lc = net.local_condition_from_audio(
                    spec, audio.reshape(audio.shape[0], -1), lengths)
            trace_step = args.store_metadata and step % 50 == 0
            trace = trace_step and rank == 0
            if trace:
                print('Storing metadata')
                prof = torch.profiler.profile(
                    activities=[torch.profiler.ProfilerActivity.CPU,
                                torch.profiler.ProfilerActivity.CUDA])
                prof.__enter__()
            loss = net.loss(input_batch=audio, global_condition_batch=gc,
                            l2_regularization_strength=l2,
                            local_condition_batch=lc,
                            local_condition_offset=lc_off,
                            lengths=lengths, loss_denominator=den)
            optimizer.minimize(loss)
            # The reference fetches the loss inside sess.run and so waits for
            # every step (train.py:300-311).  Here the step is queued on the
            # device and its loss is read ONE step later, while the next step
            # runs (the same lines, one step late; 12.0 -> 9.5 ms per step at
            # 8 x 16000: bench.py's step time) -- except where the step's own state is needed at
            # once: a checkpoint step, a traced step, the last step.
            # (the norm first: the loss's event, recorded behind both copies,
            # then covers it.  Every rank holds the same norm: no collective)
            norm = None if optimizer.last_grad_norm is None else \
                fetch_later(optimizer.last_grad_norm, step, tag=1)
            mean_loss = fetch_later(parallel.allreduce_mean_scalar(loss), step)
            if pending is not None:
                report(*pending)
            pending = (step, mean_loss, start_time, real, norm)
            if trace_step:
                report(*pending)
                pending = None
            if trace:
                prof.__exit__(None, None, None)
                prof.export_chrome_trace(os.path.join(logdir,
                                                      'timeline.trace'))
            if step % args.checkpoint_every == 0:
                # (every rank resolves the step here, so that the ranks'
                # collective sequences stay equal on the error path of report)
                if pending is not None:
                    report(*pending)
                    pending = None
            if rank == 0 and step % args.checkpoint_every == 0:
                save(net, logdir, step, optimizer, lc_entry,
                     corpus_at(step))
                last_saved_step = step
                if args.histograms:
                    # the reference's histogram summaries (model.py:314-325)
                    # as an .npz next to the checkpoint
                    hs = net.histogram_summaries()
                    np.savez(os.path.join(
                        logdir, 'histograms-%d.npz' % step),
                        **{k + '/counts': v[0] for k, v in hs.items()},
                        **{k + '/range': np.asarray(v[1:])
                           for k, v in hs.items()})
            if vset is not None:
                last_run = step
                if step % validate_every == 0:
                    # (the one-step-late training line first: the lines stay
                    # in order)
                    if pending is not None:
                        report(*pending)
                        pending = None
                    validate(step)
                    validated = step
        if pending is not None:
            report(*pending)
            pending = None
        if vset is not None and last_run is not None and \
                validated != last_run:
            validate(last_run)              # after the last step
    except KeyboardInterrupt:
        print()
    finally:
        if rank == 0 and step is not None and step > last_saved_step:
            save(net, logdir, step, optimizer, lc_entry, corpus_at(step))
        coord.request_stop()
        coord.join(threads)
        if events:
            events.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
