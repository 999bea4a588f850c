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
import collections
import json
import os
import sys
import time
from datetime import datetime

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import (  # noqa: E402
    emphasis, features, input_noise, local_condition, lpc, mol)
from wavenet.checkpoint import (  # noqa: E402,F401
    checkpoint_path, latest_checkpoint, load, open_latest, save)
from wavenet.cli import (  # noqa: E402
    PIECE_HISTORY_HELP, model_from_params, piece_history, piece_history_arg,
    str_to_bool)

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
    p.add_argument('--histograms', type=str_to_bool, default=False)
    p.add_argument('--gc_channels', type=int, default=None,
                   help='Number of global condition channels.')
    p.add_argument('--dp_overlap_allreduce', type=str_to_bool, default=False,
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
    p.add_argument('--mask_padding', type=str_to_bool, default=False,
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
    p.add_argument('--validate_ema', type=str_to_bool, default=False,
                   help='Validate the exponential moving average of the '
                        'weights instead of the weights (needs --ema_decay).')
    features.add_cli_flags(
        p, '  Needs --lc_channels and --lc_hop or --lc_upsample_scales; '
        'with --mask_padding true the clips\' lengths go to the front end '
        'too.  The settings are stored in every checkpoint (\'lc_features\') '
        'and --validation_dir is scored through the same front end.')
    p.add_argument('--device_corpus', type=str_to_bool, default=False,
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
    p.add_argument('--piece_history', type=piece_history_arg, default=None,
                   metavar='N|rf',
                   help='--device_corpus true with --sample_size: '
                        + PIECE_HISTORY_HELP + '  The loss then always gets '
                        'the clips\' lengths, the step line shows the '
                        'predicted samples, and --validation_dir is scored '
                        'with the same history.')
    emphasis.add_cli_flag(p, train=True)
    input_noise.add_cli_flags(p, train=True)
    lpc.add_cli_flags(p, train=True)
    mol.add_cli_flags(p)
    args = p.parse_args(argv)
    # ((K, log_scale_min) of --output_mixture, or None)
    args.mixture = mol.from_cli(p, args)
    if lpc.flag_error(args, 'train'):
        p.error(lpc.flag_error(args, 'train'))
    # (the InputNoise of --input_noise, or None)
    args.noise = input_noise.from_cli(p, args)
    if args.preemphasis is not None:
        try:
            emphasis.Emphasis(args.preemphasis)
        except ValueError as e:
            p.error('--preemphasis: %s' % e)
    # (--data_dir's default is filled in here, so that "not given" shows)
    data_dir_given = args.data_dir is not None
    if not data_dir_given:
        args.data_dir = DATA_DIRECTORY
    if args.device_corpus:
        if not data_dir_given:
            p.error('--device_corpus true needs --data_dir')
        if args.synthetic:
            p.error('--device_corpus true does not go with --synthetic')
        if args.lc_channels is not None and \
                args.lc_features not in features.KINDS:
            p.error('--device_corpus true reads no <clip>.npy features: '
                    '--lc_channels needs --lc_features mel or mel+f0 with '
                    'it')
        if args.crop == 'random' and not args.sample_size:
            p.error('--crop random needs --sample_size')
    elif args.crop is not None:
        p.error('--crop needs --device_corpus true')
    if args.piece_history is not None:
        missing = [flag for flag, given in (
            ('--device_corpus true', args.device_corpus),
            ('--sample_size', bool(args.sample_size))) if not given]
        if missing:
            p.error('--piece_history needs %s' % ' and '.join(missing))
    if args.lc_feature_context == 'utterance' and not (
            args.device_corpus and args.lc_features in features.KINDS):
        p.error('--lc_feature_context utterance needs --device_corpus true '
                'and --lc_features mel or mel+f0')
    if args.lc_feature_context is not None and \
            args.lc_features not in features.KINDS:
        p.error('--lc_feature_context needs --lc_features mel or mel+f0')
    if features.f0_flags_refused(args):
        p.error(features.f0_flags_refused(args))
    if args.lc_features in features.KINDS:
        if args.lc_channels is None:
            p.error('--lc_features %s needs --lc_channels (the number of '
                    'mels%s)' % (args.lc_features, ' + 2' if
                                 args.lc_features == 'mel+f0' else ''))
        if args.lc_hop is None and args.lc_upsample_scales is None:
            p.error('--lc_features %s needs --lc_hop or '
                    '--lc_upsample_scales (hop = their product)'
                    % args.lc_features)
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


def corpus_first_batch(stored, entry):
    """--device_corpus: step k of a run takes batch base + k.  A run continued
    in its logdir continues its step count (base 0).  A new training restored
    from a checkpoint starts at step 0: it goes on with the batch after the
    last one of the checkpoint's 'device_corpus' entry `stored` where that
    has this run's settings `entry`, else it starts the sequence again."""
    if stored is None:
        return 0
    # ('history' is not compared: the pieces' sequence does not depend on it)
    same = [k for k in entry if k != 'history']
    if {k: stored.get(k) for k in same} != {k: entry[k] for k in same}:
        print("  The checkpoint's corpus settings {} differ: the corpus "
              "starts again.".format(stored))
        return 0
    base = int(stored.get('batch', -1)) + 1
    print('  Corpus batches continue at {}.'.format(base))
    return base


def emphasis_from_flags(args, opened, continued):
    """The Emphasis of --preemphasis and the restored checkpoint's 'emphasis'
    entry (`opened`: checkpoint.open_latest's result), or None: the entry is
    the default, the flag overrides it (0: off) -- but a run `continued` in
    its logdir keeps its checkpoint's value: ValueError naming both."""
    stored = None
    if opened is not None and opened.ckpt is not None:
        stored = opened.ckpt.get('emphasis')
    else:
        continued = False       # (nothing to continue, or not our format)
    return emphasis.from_cli(args.preemphasis, stored, continued)


def lpc_from_flags(args, spec, opened, continued):
    """The LinearPrediction of the --lpc_* flags and the restored
    checkpoint's 'lpc' entry over the front end `spec`, or None; as
    emphasis_from_flags."""
    stored = None
    if opened is not None and opened.ckpt is not None:
        stored = opened.ckpt.get('lpc')
    else:
        continued = False
    return lpc.from_cli(args, spec, stored, continued)


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


FrontEnd = collections.namedtuple('FrontEnd',
                                  'spec kept_norm lc_stats from_corpus')


def front_end_from_flags(args, sample_rate, lc_hop, continued):
    """--lc_features, before the corpus exists: FrontEnd(the MelSpec of the
    flags or None, the normaliser kept from the checkpoint or None, the sums
    of --lc_stats or None, whether the corpus has to supply the statistics).
    `continued`: checkpoint.open_latest's result for a run that continues in
    its logdir, else None.  ValueError / OSError: flags that do not fit.

    The normaliser, by --lc_normalize, --lc_stats, a continued run whose
    checkpoint stores a normaliser, and --lc_feature_context:

      normalize     stats  continued  context    the spec's normaliser
      none / range  -      any        any        none / the range; nothing is
                                                 kept, nothing is summed
      absent        -      no         any        none
      absent        -      yes        any        the checkpoint's (*)
      corpus        FILE   no         any        from FILE
      corpus        FILE   yes        any        the checkpoint's (*)
      corpus        -      no         utterance  the corpus sums its resident
                                                 frames at load and
                                                 normalises them in place
      corpus        -      no         piece      from one pass over the
                                                 utterances
      corpus        -      yes        utterance  the checkpoint's (*), applied
                                                 to the resident frames; their
                                                 sums are compared with it
                                                 ("... differ ... is kept")
      corpus        -      yes        piece      the checkpoint's (*); no pass

    (*) prints "The checkpoint's feature normaliser continues."  The last
    four rows are decided in front_end_from_corpus.  <logdir>/lc_stats.npz
    is written wherever sums exist: FILE's, or the corpus's (every `corpus -`
    row but the last)."""
    spec = features.spec_from_cli(args, sample_rate, args.lc_channels, lc_hop,
                                  corpus=args.device_corpus)
    lc_stats = features.FeatureStats.load(args.lc_stats) \
        if spec is not None and args.lc_stats is not None else None
    kept_norm = None
    if spec is not None and continued is not None and \
            continued.ckpt is not None and \
            args.lc_normalize in (None, 'corpus'):
        kept = (continued.ckpt.get('lc_features') or {}).get('normalizer')
        if kept is not None:
            kept_norm = features.Normalizer.from_entry(kept)
            print('  The checkpoint\'s feature normaliser continues.')
            spec = spec.with_normalizer(kept_norm)
    from_corpus = spec is not None and args.lc_normalize == 'corpus' and \
        args.lc_stats is None
    return FrontEnd(spec, kept_norm, lc_stats, from_corpus)


def stats_allreduce(front, world):
    """How the corpus sums its feature statistics over the ranks, or None."""
    if not (front.from_corpus and world > 1):
        return None
    from wavenet import parallel
    return lambda v: parallel.sum_float64_over_ranks(
        v, 'cuda' if torch.cuda.is_available() else 'cpu')


def open_corpus(args, wavenet_params, front, rank, world):
    """--device_corpus: the corpus on the device replaces the reader and its
    threads for the training batches (wavenet/corpus.py)."""
    from wavenet.corpus import DeviceCorpus
    utt_ctx = args.lc_feature_context == 'utterance'
    corpus_norm = {}
    if utt_ctx and front.from_corpus:
        # the resident frames: summed and normalised in place at load
        stats_sum = stats_allreduce(front, world)
        corpus_norm = \
            dict(normalize=front.kept_norm, stats_allreduce=stats_sum) \
            if front.kept_norm is not None else \
            dict(normalize='corpus', normalize_clip=args.lc_norm_clip,
                 stats_allreduce=stats_sum)
    return DeviceCorpus(
        args.data_dir, wavenet_params['sample_rate'],
        args.gc_channels is not None, sample_size=args.sample_size or None,
        silence_threshold=args.silence_threshold,
        crop=args.crop or 'pieces', seed=CORPUS_SEED, rank=rank, world=world,
        spec=front.spec if utt_ctx else None,
        history=piece_history(args.piece_history, wavenet_params),
        **corpus_norm)


def front_end_from_corpus(args, front, corpus, world):
    """--lc_features, once the corpus is loaded: (spec, lc_stats) with the
    corpus's statistics where it has to supply them
    (front_end_from_flags's table)."""
    spec, kept_norm, lc_stats, from_corpus = front
    if not from_corpus:
        return spec, lc_stats
    if args.lc_feature_context == 'utterance':
        lc_stats, spec = corpus.feature_stats, corpus.spec
    elif kept_norm is None:
        # no frames are resident: one pass over the utterances
        lc_stats = corpus.compute_feature_stats(
            spec, stats_allreduce(front, world))
    if kept_norm is None:
        spec = spec.with_normalizer(features.Normalizer.from_stats(
            lc_stats, args.lc_norm_clip))
    elif lc_stats is not None:
        fresh = features.Normalizer.from_stats(lc_stats)
        if not (np.array_equal(fresh.shift, kept_norm.shift) and
                np.array_equal(fresh.scale, kept_norm.scale)):
            print('  The corpus\'s feature statistics differ from '
                  'the checkpoint\'s normaliser, which is kept.')
    return spec, lc_stats


def corpus_settings(args, history=0):
    """What a checkpoint's 'device_corpus' entry says about the corpus
    ('history': only where there is some; the sequence of pieces does not
    depend on it)."""
    entry = dict(crop=args.crop or 'pieces', seed=CORPUS_SEED,
                 sample_size=args.sample_size or None,
                 lc_feature_context=args.lc_feature_context or 'piece')
    if history:
        entry['history'] = int(history)
    return entry


def build_source(args, wavenet_params, front, file_lc, lc_scales, lc_hop,
                 rank, world, emph=None):
    """The training batches' source (wavenet/training.py) and the front end
    as it stands once the source exists: (source, spec, lc_stats) -- or None,
    having printed why not.  file_lc: the channels of <clip>.npy features;
    emph: the Emphasis the source applies to every batch, or None."""
    from wavenet import AudioReader, training
    from wavenet.audio_reader import Coordinator
    gc_enabled = args.gc_channels is not None
    # what the source yields beside the audio: the files' features ...
    lc_mode = None if file_lc is None else \
        'frames' if lc_scales is not None else 'rows'
    if args.device_corpus:
        try:
            corpus = open_corpus(args, wavenet_params, front, rank, world)
        except (ValueError, MemoryError) as e:
            print(str(e))
            return None
        spec, lc_stats = front_end_from_corpus(args, front, corpus, world)
        # ... or the utterances' frames, which the corpus holds
        if args.lc_feature_context == 'utterance':
            lc_mode = 'frames' if lc_scales is not None else 'rows'
        return training.CorpusSource(
            corpus, corpus_settings(args, corpus.index.history),
            args.mask_padding, gc_enabled,
            lc_mode, emphasis=emph), spec, lc_stats
    coord = Coordinator()
    if args.synthetic:
        reader = SyntheticReader(
            args.sample_size, args.gc_cardinality if gc_enabled else None,
            rank=rank, lc_channels=file_lc, lc_hop=lc_hop or 1)
    else:
        if args.lc_channels is not None and not lc_hop:
            print('--lc_channels needs --lc_hop (audio samples per feature '
                  'frame)')
            return None
        # The reference computes `silence_threshold = None if below EPSILON`
        # and then passes the RAW flag to the reader (train.py:211-220; SURVEY
        # Appendix A: "do not fix silently") -- same here:
        # `--silence_threshold 0` trims with a threshold of 0 (only exactly
        # silent frames go) instead of skipping the trimming.
        reader = AudioReader(
            args.data_dir, coord, sample_rate=wavenet_params['sample_rate'],
            gc_enabled=gc_enabled, sample_size=args.sample_size,
            silence_threshold=args.silence_threshold, rank=rank, world=world,
            seed=rank, lc_channels=file_lc, lc_hop=lc_hop,
            lc_frames=lc_scales is not None)
    return training.ReaderSource(reader, coord, args.mask_padding, gc_enabled,
                                 lc_mode, emphasis=emph), front.spec, \
        front.lc_stats


def save_histograms(net, logdir, step):
    """The reference's histogram summaries (model.py:314-325) as an .npz next
    to the checkpoint."""
    hs = net.histogram_summaries()
    np.savez(os.path.join(logdir, 'histograms-%d.npz' % step),
             **{k + '/counts': v[0] for k, v in hs.items()},
             **{k + '/range': np.asarray(v[1:]) for k, v in hs.items()})


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

    from wavenet import optimizer_factory, parallel, training
    rank, world, local = parallel.init_from_env(host_control_plane=True)
    if torch.cuda.is_available():
        torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))

    with open(args.wavenet_params, 'r') as f:
        wavenet_params = json.load(f)
    sample_rate = wavenet_params['sample_rate']
    noise = args.noise
    if noise is not None and wavenet_params.get('scalar_input'):
        print('--input_noise is not for scalar_input models: their network '
              'input is the float audio, not the codes')
        return 1
    # (read once: the front end below and load() share it)
    opened = open_latest(restore_from)

    gc_enabled = args.gc_channels is not None
    # --lc_features: the sources yield audio only, the features of every
    # batch are computed on the device (by the loop from the batch as cut,
    # by the corpus from the whole utterance).  A run continued in its logdir
    # keeps the normaliser of its checkpoint.
    try:
        front = front_end_from_flags(
            args, sample_rate, lc_hop,
            None if is_overwritten_training else opened)
        emph = emphasis_from_flags(args, opened, not is_overwritten_training)
    except (ValueError, OSError) as e:
        print(str(e))
        return 1
    # (with a front end the readers yield audio only)
    file_lc = None if front.spec is not None else args.lc_channels
    built = build_source(args, wavenet_params, front, file_lc, lc_scales,
                         lc_hop, rank, world, emph)
    if built is None:
        return 1
    source, spec, lc_stats = built
    try:
        lp = lpc_from_flags(args, spec, opened, not is_overwritten_training)
    except ValueError as e:
        print(str(e))
        return 1
    source.lpc = lp
    # (the one place that decides what lc is: the source's, or the front
    # end's of the batch as the source cut it)
    lc_from_batch = spec is not None and source.lc is None

    lc_entry = None if spec is None else features.checkpoint_entry(spec)
    emph_entry = None if emph is None else emph.entry()
    if emph is not None:
        print('  Training on the pre-emphasised signal, alpha = {!r}.'
              .format(emph.alpha))
    lpc_entry = None if lp is None else lp.entry()
    output_entry = None if args.mixture is None else \
        mol.output_entry(*args.mixture)
    if opened is not None and opened.ckpt is not None:
        # (a checkpoint trained with another head holds variables of another
        # shape)
        try:
            mol.same_entry(opened.ckpt.get('output'),
                           *(args.mixture or (None, None)))
        except ValueError as e:
            print(str(e))
            return 1
    if args.mixture is not None:
        print('  Training a mixture of {} logistics over 65536 levels '
              '(log scale floor {!r}).'.format(*args.mixture))
    if lp is not None:
        print('  Training on the linear-prediction excitation: {!r}.'
              .format(lp))
    noise_entry = None if noise is None else noise.entry()
    if noise is not None:
        print('  Training on perturbed input codes (clean targets): '
              'probability {!r}, width {}, seed {}.'
              .format(noise.prob, noise.width, noise.seed))
    if lc_stats is not None and rank == 0:
        os.makedirs(logdir, exist_ok=True)
        lc_stats.save(os.path.join(logdir, 'lc_stats.npz'))

    net = model_from_params(
        wavenet_params, args.batch_size, histograms=args.histograms,
        global_condition_channels=args.gc_channels,
        global_condition_cardinality=source.gc_category_cardinality,
        local_condition_channels=args.lc_channels,
        local_condition_upsample_scales=lc_scales,
        local_condition_context=lc_ctx, **mol.model_keywords(args.mixture))
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
        saved_global_step = load(net, restore_from, optimizer, restored,
                                 opened)
        if is_overwritten_training or saved_global_step is None:
            # the first training step will be saved_global_step + 1
            saved_global_step = -1
        if args.device_corpus and is_overwritten_training:
            source.base = corpus_first_batch(restored.get('device_corpus'),
                                             source.entry)
    except Exception:
        print("Something went wrong while restoring checkpoint. "
              "We will terminate training to avoid accidentally overwriting "
              "the previous model.")
        raise
    del opened                  # (the checkpoint's tensors)
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
            args.validation_dir, sample_rate, sample_size=args.sample_size,
            silence_threshold=args.silence_threshold, gc_enabled=gc_enabled,
            gc_cardinality=source.gc_category_cardinality,
            lc_channels=file_lc, lc_hop=lc_hop,
            lc_frames=lc_scales is not None, rank=rank, world=world,
            history=piece_history(args.piece_history, wavenet_params)
            if args.sample_size else 0)
    validate_every = args.validate_every or args.checkpoint_every

    if lc_from_batch:
        # the front end's features of the raw batch as the source cut it:
        # frames (offset 0) for an upsampler model, else rows
        source.front = lambda audio, n: net.local_condition_from_audio(
            spec, audio, n)
    source.start(net.device)
    log = training.StepLog(net, logdir, rank)
    B = args.batch_size
    step = None
    last_saved_step = saved_global_step
    last_run = validated = None   # --validation_dir: last step run / validated
    try:
        for step in range(saved_global_step + 1, args.num_steps):
            start_time = time.time()
            # every rank takes the same decision for this step (skip / common
            # clip length / abort) BEFORE any collective of the step is issued
            err = None
            try:
                T, lengths, gc = source.plan(step, B)
            except Exception as e:        # e.g. a reader-thread failure
                err, T, lengths, gc = e, 0, None, None
            n_t, all_ok = parallel.agree_step(T, err is None, net.device)
            if not all_ok:
                raise RuntimeError('rank %d: a rank failed to produce a batch '
                                   'at step %d%s' % (rank, step, '' if err is
                                                     None else ': %r' % err))
            den = real = hist = None
            if lengths is not None:
                # (cut to the common T like the rows; every rank's longest
                # real clip is then n_t samples, so the guard below looks at
                # the longest real length and decides the same on every rank)
                lengths = np.minimum(lengths, n_t)
                # (--piece_history: a clip cut to its history or less has
                # no target; the real samples are the predicted ones)
                hist = source.history(step, B, n_t)
                den = parallel.masked_denominator(lengths, net.device,
                                                  history=hist)
                real = int(round(den * world))
            if (n_t if lengths is None else int(lengths.max())) < 2 or \
                    den == 0:
                continue
            audio, lc, lc_off = source.take(step, B, n_t, lengths)
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
                            lengths=lengths, loss_denominator=den,
                            **({} if hist is None else dict(history=hist)),
                            **({} if noise is None else dict(
                                input_noise=noise,
                                noise_keys=input_noise.step_keys(
                                    step, B, rank, world))))
            optimizer.minimize(loss)
            # (prints the step before: StepLog)
            log.step(step, loss, optimizer.last_grad_norm, start_time, real)
            if trace_step:
                log.flush()
            if trace:
                prof.__exit__(None, None, None)
                prof.export_chrome_trace(os.path.join(logdir,
                                                      'timeline.trace'))
            if step % args.checkpoint_every == 0:
                # (every rank resolves the step here, so that the ranks'
                # collective sequences stay equal on the error path of the
                # report)
                log.flush()
            if rank == 0 and step % args.checkpoint_every == 0:
                save(net, logdir, step, optimizer, lc_entry,
                     source.checkpoint_entry(step), emph_entry,
                     noise_entry, lpc_entry, output_entry)
                last_saved_step = step
                if args.histograms:
                    save_histograms(net, logdir, step)
            if vset is not None:
                last_run = step
                if step % validate_every == 0:
                    # (the one-step-late training line first: the lines stay
                    # in order)
                    log.flush()
                    log.validation(step, training.validate(
                        net, optimizer, vset, spec, args, emph, lp))
                    validated = step
        log.flush()
        if vset is not None and last_run is not None and \
                validated != last_run:
            # after the last step
            log.validation(last_run, training.validate(
                net, optimizer, vset, spec, args, emph, lp))
    except KeyboardInterrupt:
        print()
    finally:
        if rank == 0 and step is not None and step > last_saved_step:
            save(net, logdir, step, optimizer, lc_entry,
                 source.checkpoint_entry(step), emph_entry,
                 noise_entry, lpc_entry, output_entry)
        source.stop()
        log.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
