#!/usr/bin/env python
"""Generation script: MI355X counterpart of the reference's generate.py.

Same flags and defaults (generate.py:38-116); the per-sample
`sess.run` loop of the reference (generate.py:213-241) is one persistent HIP
kernel (`WaveNetModel.generate`): priming with a --wav_seed (generate.py:195-210,
one step per seed sample) and temperature sampling happen on the device.
--fast_generation false uses the windowed naive path (`predict_proba`, host-side
np.random.choice) like the reference.  wav I/O is scipy (librosa is absent).

Local conditioning: --lc_path features.npy [frames, Lc] are upsampled by
repetition (--lc_hop samples per frame) and ONE sample is generated per
upsampled row after the seed (--samples is ignored).  Row k sits beside
generated sample k, as in training (the row beside input sample t conditions
the prediction of sample t + 1); the seed's rows are zeros.  On the naive path
(--fast_generation false) each window passes its own rows to predict_proba.
--lc_fast_generation true opts in to fast generation instead: `generate` /
`continue_generation` (in --save_every chunks) take the rows of the positions
they step through, and with --clips N `generate_batch` runs the N clips on
rows shared by all of them.  Without either flag --lc_path is refused.
With --lc_upsample_scales (a model trained with train.py
--lc_upsample_scales) the frames are upsampled once by the checkpoint's
learned network (`upsample_local_condition`) instead of by repetition; the
flows above then run on those rows.  --lc_context P (a model trained with
train.py --lc_context P) applies the checkpoint's frame-context convolution in
front of that upsampler.
--lc_wav in.wav takes the place of --lc_path (copy synthesis): the features
are the log-mel front end's (wavenet/features.py) of that wav, computed on the
device with the checkpoint's 'lc_features' settings (train.py --lc_features)
or the --lc_features flags; one sample is generated per sample of the wav, or
--samples of them when that is given and fewer.
--lc_wav_dir DIR --wav_out_dir OUT is --lc_wav for every wav of a directory
(sorted; file i draws with --seed + i): --clips streams (default 32 here) run
in lock step, the utterances sorted by length (wavenet/synthesis.py), and
OUT/<stem>.wav holds one generated sample per sample of DIR/<stem>.wav.
--synthesis_schedule queue refills a finished stream's slot with the next
utterance at once instead of running length-sorted rounds: the same files in
fewer lock-step steps.
Pre-emphasis: a model trained with train.py --preemphasis generates the
emphasised signal; what is decoded goes through the inverse filter on the
device before it is written (the checkpoint's 'emphasis' entry, or
--preemphasis A; 0: off), and a --wav_seed is pre-emphasised before it is
encoded.  generated_codes.npy holds the model's codes as they are.
Linear prediction: a model trained with train.py --lpc_order generates the
prediction residual; what is decoded behind the seed goes through the
all-pole filter of every frame on the device before it is written (the
checkpoint's 'lpc' entry, or --lpc_order P and its value flags; 0: off).  The
coefficients come from the raw log-mel frames that condition the run: those
of --lc_wav / --lc_wav_dir, or --lc_path's with the checkpoint's normaliser
inverted (what the normaliser clamped stays clamped).  Without frames there
is no filter: such a run is refused.
Mixture-of-logistics checkpoints (train.py --output_mixture) generate on the
naive path (--fast_generation false), or with --fast_mixture true on the
batched generator (`generate_mixture`; --clips N: `generate_mixture_batch`,
clip i drawing with --seed + i), in --save_every chunks through
`continue_mixture`.  Both write a 16-bit wav and generated_levels.npy.  The
draw's counter is the stream's step, the seed's steps included, so the two
paths draw the same numbers only from a one-sample seed.
"""
from __future__ import division
from __future__ import print_function

import argparse
import json
import os
import sys
from datetime import datetime

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
from wavenet import (  # noqa: E402
    emphasis, features, local_condition, lpc, mol, sampling)
from wavenet.checkpoint import (  # noqa: E402,F401
    context_mismatch, open_ema_checkpoint, restore, stored_emphasis, stored_lpc,
    stored_output,
    stored_lc_features, upsampler_mismatch)
from wavenet.cli import model_from_params, str_to_bool  # noqa: E402

SAMPLES = 16000
TEMPERATURE = 1.0
LOGDIR = './logdir'
WINDOW = 8000
WAVENET_PARAMS = './wavenet_params.json'
SAVE_EVERY = None
SILENCE_THRESHOLD = 0.1
DIR_CLIPS = 32


def _ensure_positive_float(f):
    if float(f) <= 0:
        raise argparse.ArgumentTypeError('Argument must be greater than zero')
    return float(f)


def _top_k(v):
    try:
        k = int(v)
    except ValueError:
        k = 0
    if k < 1:
        raise argparse.ArgumentTypeError('Argument must be an integer >= 1')
    return k


def _top_p(v):
    try:
        f = float(v)
    except ValueError:
        f = float('nan')
    if not (np.isfinite(f) and 0.0 < f <= 1.0):
        raise argparse.ArgumentTypeError('Argument must be in (0, 1]')
    return f


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description='WaveNet generation script')
    p.add_argument('checkpoint', type=str,
                   help='Which model checkpoint to generate from')
    p.add_argument('--samples', type=int, default=None,
                   help='samples to generate (default %d; with --lc_wav: '
                   'the length of that wav)' % SAMPLES)
    p.add_argument('--temperature', type=_ensure_positive_float,
                   default=TEMPERATURE)
    p.add_argument('--top_k', type=_top_k, default=None,
                   help='draw from the K most probable codes only (ties at '
                   'the cut are kept)')
    p.add_argument('--top_p', type=_top_p, default=None,
                   help='draw from the nucleus only: the most probable codes '
                   'that hold this share of the tempered distribution')
    p.add_argument('--logdir', type=str, default=LOGDIR)
    p.add_argument('--window', type=int, default=WINDOW,
                   help='Past samples taken into account per step (naive '
                   'path) / kept of the seed')
    p.add_argument('--wavenet_params', type=str, default=WAVENET_PARAMS)
    p.add_argument('--wav_out_path', type=str, default=None)
    p.add_argument('--save_every', type=int, default=SAVE_EVERY)
    p.add_argument('--fast_generation', type=str_to_bool, default=True)
    p.add_argument('--fast_mixture', type=str_to_bool, default=False,
                   help='a mixture-of-logistics checkpoint: generate on the '
                   'batched generator (generate_mixture / '
                   'generate_mixture_batch) instead of the naive path '
                   '(default false: such a checkpoint needs '
                   '--fast_generation false)')
    p.add_argument('--wav_seed', type=str, default=None)
    p.add_argument('--gc_channels', type=int, default=None)
    p.add_argument('--gc_cardinality', type=int, default=None)
    p.add_argument('--gc_id', type=int, default=None)
    p.add_argument('--seed', type=int, default=0, help='sampling RNG seed')
    p.add_argument('--clips', type=int, default=None,
                   help='independent clips generated together (fast path); '
                   'clip i draws with --seed + i and is written to '
                   '<stem>_<i><ext> (default 1; with --lc_wav_dir: the '
                   'streams per round, default %d)' % DIR_CLIPS)
    p.add_argument('--lc_path', type=str, default=None,
                   help='local conditioning features (.npy, [frames, '
                   'channels]); needs --fast_generation false or '
                   '--lc_fast_generation true')
    p.add_argument('--lc_fast_generation', type=str_to_bool, default=False,
                   help='with --lc_path: generate on the fast path '
                   '(default false: --lc_path needs --fast_generation false)')
    p.add_argument('--lc_hop', type=int, default=1,
                   help='audio samples per feature frame of --lc_path')
    p.add_argument('--lc_upsample_scales', type=str, default=None,
                   help='with --lc_path: the scales of the model\'s learned '
                   'upsampler (train.py --lc_upsample_scales), e.g. 4,5,10')
    p.add_argument('--lc_context', type=int, default=None,
                   help='with --lc_upsample_scales: P of the model\'s '
                   'frame-context convolution (train.py --lc_context)')
    p.add_argument('--gc_ids', type=str, default=None,
                   help='comma-separated global condition ids, one clip each '
                   '(sets --clips to their number)')
    p.add_argument('--use_ema', type=str_to_bool, default=False,
                   help='generate from the checkpoint\'s exponential moving '
                   'average of the weights (train.py --ema_decay)')
    p.add_argument('--lc_wav', type=str, default=None,
                   help='local conditioning from a wav: its log-mel '
                   'features, computed on the device, take the place of '
                   '--lc_path (not both)')
    p.add_argument('--lc_wav_dir', type=str, default=None,
                   help='--lc_wav for every wav of this directory, --clips '
                   'at a time; needs --wav_out_dir (not with --lc_wav or '
                   '--lc_path)')
    p.add_argument('--synthesis_schedule', type=str, default=None,
                   choices=('rounds', 'queue'),
                   help='with --lc_wav_dir: length-sorted rounds (the '
                   'default), or the restart queue, in which a finished '
                   'stream\'s slot takes the next utterance at once')
    p.add_argument('--wav_out_dir', type=str, default=None,
                   help='with --lc_wav_dir: the directory of the generated '
                   '<stem>.wav files')
    p.add_argument('--lc_channels', type=int, default=None,
                   help='with --lc_wav: the number of mels (default: the '
                   'checkpoint\'s)')
    features.add_cli_flags(
        p, '  With --lc_wav; default: the checkpoint\'s \'lc_features\' '
        '(train.py --lc_features), whose settings the other --lc_* flags '
        'default to.')
    emphasis.add_cli_flag(p)
    lpc.add_cli_flags(p)
    a = p.parse_args(argv)
    if lpc.flag_error(a, 'generate'):
        p.error(lpc.flag_error(a, 'generate'))
    if a.preemphasis is not None:
        try:
            emphasis.Emphasis(a.preemphasis)
        except ValueError as e:
            p.error('--preemphasis: %s' % e)
    if a.fast_mixture:
        if not a.fast_generation:
            p.error('--fast_mixture true is a fast path: it does not go with '
                    '--fast_generation false')
        if a.top_k is not None or a.top_p is not None:
            p.error('--fast_mixture true: --top_k / --top_p truncate a '
                    'distribution over codes; a mixture\'s draw has none '
                    '(use --temperature)')
        if a.lc_wav_dir is not None:
            p.error('--fast_mixture true does not go with --lc_wav_dir: bulk '
                    'synthesis for mixture checkpoints is a follow-up')
    if a.lc_wav is not None and a.lc_path is not None:
        p.error('give either --lc_wav or --lc_path, not both')
    if a.lc_wav_dir is not None:
        for other in ('lc_wav', 'lc_path'):
            if getattr(a, other) is not None:
                p.error('give either --lc_wav_dir or --%s, not both' % other)
        if a.wav_out_dir is None:
            p.error('--lc_wav_dir needs --wav_out_dir')
        if a.gc_ids is not None:
            p.error('--gc_ids does not go with --lc_wav_dir (one --gc_id '
                    'for all files)')
        if a.clips is None:
            a.clips = DIR_CLIPS
        if not 1 <= a.clips <= 256:
            p.error('--clips must be in [1, 256] with --lc_wav_dir')
    elif a.wav_out_dir is not None:
        p.error('--wav_out_dir needs --lc_wav_dir')
    elif a.synthesis_schedule is not None:
        p.error('--synthesis_schedule needs --lc_wav_dir')
    if a.clips is None:
        a.clips = 1
    if a.lc_wav is None and a.lc_wav_dir is None:
        for flag in ['--lc_features'] * (a.lc_features in features.KINDS) + \
                features.cli_flags_given(a) + features.f0_flags_given(a):
            p.error('%s needs --lc_wav' % flag)
    elif a.lc_features == 'none':
        p.error('--lc_wav needs a front end, not --lc_features none')
    if features.f0_flags_refused(a, stored_may_decide=True):
        p.error(features.f0_flags_refused(a, stored_may_decide=True))
    if a.lc_wav_dir is not None and not a.fast_generation:
        p.error('--lc_wav_dir runs on the fast path only')
    a.samples_given = a.samples is not None
    if a.samples is None:
        a.samples = SAMPLES
    if a.gc_ids is not None:
        a.gc_ids = [int(v) for v in a.gc_ids.split(',') if v.strip()]
        if not a.gc_ids:
            raise ValueError('--gc_ids needs at least one id')
        if a.clips not in (1, len(a.gc_ids)):
            raise ValueError('--clips {} does not match the {} ids of --gc_ids'
                             .format(a.clips, len(a.gc_ids)))
        if a.gc_id is not None:
            raise ValueError('give either --gc_id or --gc_ids')
        a.clips = len(a.gc_ids)
        if len(a.gc_ids) == 1:
            a.gc_id, a.gc_ids = a.gc_ids[0], None
    if a.clips < 1:
        raise ValueError('--clips must be >= 1')
    if a.clips > 1 and not a.fast_generation and a.lc_wav_dir is None:
        raise ValueError('--clips > 1 needs --fast_generation true')
    if a.gc_channels is not None:
        if a.gc_cardinality is None:
            raise ValueError("Globally conditioning but gc_cardinality not "
                             "specified. Use --gc_cardinality=377 for full "
                             "VCTK corpus.")
        if a.gc_id is None and a.gc_ids is None:
            raise ValueError("Globally conditioning, but global condition was "
                             "not specified. Use --gc_id to specify global "
                             "condition.")
    return a


def write_wav(waveform, sample_rate, filename):
    from scipy.io import wavfile
    wavfile.write(filename, int(sample_rate),
                  np.asarray(waveform, dtype=np.float32))
    print('Updated wav file at {}'.format(filename))


def write_wav16(waveform, sample_rate, filename):
    """16-bit PCM: sample x becomes its level (wavenet/mol.py's rule) minus
    32768, so a waveform of level centres is written without loss."""
    from scipy.io import wavfile
    lv, _ = mol.levels_reference(np.asarray(waveform, np.float32))
    wavfile.write(filename, int(sample_rate),
                  (lv.astype(np.int32) - 32768).astype(np.int16))
    print('Updated wav file at {}'.format(filename))


def _mixture_seed(args, sample_rate, emph):
    """A mixture-of-logistics model's seed as float samples on the 16-bit
    grid: --wav_seed's (silence-trimmed, pre-emphasised where the model was
    trained so, cut to the window), else one level drawn with --seed."""
    if args.wav_seed:
        from wavenet.audio_reader import load_wav, trim_silence
        audio = trim_silence(load_wav(args.wav_seed, sample_rate),
                             SILENCE_THRESHOLD)
        audio = np.asarray(audio, np.float32).reshape(-1)
        if emph is not None and audio.shape[0]:
            audio = emph.pre(audio).cpu().numpy()
        audio = audio[:args.window]
    else:
        audio = None
    if audio is None or audio.shape[0] == 0:
        lv = np.random.default_rng(args.seed).integers(mol.LEVELS, size=(1,))
        return mol.centres(lv).tolist()
    return mol.levels_reference(audio)[1].tolist()


def create_seed(filename, sample_rate, quantization_channels,
                window_size=WINDOW, silence_threshold=SILENCE_THRESHOLD,
                emph=None):
    """mu-law codes of the (silence-trimmed) seed wav, pre-emphasised where
    the model was trained so (`emph`), cut to the window."""
    from wavenet import mu_law_encode
    from wavenet.audio_reader import load_wav, trim_silence
    audio = trim_silence(load_wav(filename, sample_rate), silence_threshold)
    if emph is not None and audio.shape[0]:
        audio = emph.pre(np.asarray(audio, np.float32).reshape(-1)
                         ).cpu().numpy()
    quantized = mu_law_encode(audio, quantization_channels)
    return quantized[:min(int(quantized.numel()), window_size)]


def main(argv=None):
    args = get_arguments(argv)
    ckpt = None
    if args.use_ema:
        # (before any model is built: a checkpoint without EMA weights is
        # refused whatever else the command line asks for)
        ckpt, why = open_ema_checkpoint(args.checkpoint)
        if why:
            print(why)
            return 1
    lc_rows, lc_scales, lc_ctx = None, None, None
    try:
        emph = emphasis.from_cli(args.preemphasis,
                                 stored_emphasis(args.checkpoint, ckpt))
        # (K, log_scale_min) of a checkpoint trained with --output_mixture
        head = mol.check_entry(stored_output(args.checkpoint, ckpt))
    except ValueError as e:
        print(str(e))
        return 1
    if head is None and args.fast_mixture:
        print('--fast_mixture true: the checkpoint holds a softmax model, not '
              'a mixture-of-logistics one (generate it without the flag)')
        return 1
    if head is not None:
        why = None
        if args.fast_generation and args.fast_mixture:
            pass
        elif args.fast_generation:
            why = ('--fast_generation true: the checkpoint holds a mixture-'
                   'of-logistics model; ' + mol.FOLLOW_UP)
        elif args.top_k is not None or args.top_p is not None:
            why = ('--top_k / --top_p truncate a distribution over codes; '
                   'the checkpoint holds a mixture-of-logistics model, whose '
                   'draw has none (use --temperature)')
        if why:
            print(why)
            return 1
    # linear prediction: on by the flag or by the checkpoint's entry
    lpc_stored = stored_lpc(args.checkpoint, ckpt)
    lpc_on = (args.lpc_order if args.lpc_order is not None else
              (lpc_stored or {}).get('order', 0)) != 0
    if lpc_on:
        why = None
        if emph is not None:
            why = ('--lpc_order and --preemphasis are two shaping filters '
                   '(the checkpoint\'s entries count): choose one')
        elif args.wav_seed:
            why = ('--lpc_order (or the checkpoint\'s \'lpc\' entry) does '
                   'not go with --wav_seed: a seed has no frames to take its '
                   'filter from (--lpc_order 0 switches the filter off)')
        elif args.lc_path is None and args.lc_wav is None and \
                args.lc_wav_dir is None:
            why = ('--lpc_order (or the checkpoint\'s \'lpc\' entry): the '
                   'all-pole filter needs frames: give --lc_wav, --lc_wav_dir '
                   'or --lc_path (--lpc_order 0 switches the filter off)')
        if why:
            print(why)
            return 1
    lp = lp_cf = None
    with open(args.wavenet_params, 'r') as f:
        wavenet_params = json.load(f)
    n_wav = None
    if args.lc_path is not None or args.lc_wav is not None or \
            args.lc_wav_dir is not None:
        try:
            # (--lc_hop 1, the default, counts as absent)
            lc_scales, hop, lc_ctx = local_condition.parse_cli(
                args.lc_upsample_scales, None if args.lc_hop == 1 else
                args.lc_hop, args.lc_context)
        except ValueError as e:
            print(str(e))
            return 1
    if args.lc_wav is not None or args.lc_wav_dir is not None:
        # (the hop is the model's: the scales' product, else --lc_hop, else
        # the checkpoint's)
        try:
            spec = features.spec_from_cli(
                args, wavenet_params['sample_rate'], args.lc_channels, hop,
                stored_lc_features(args.checkpoint, ckpt))
            if spec is None:
                raise ValueError(
                    '--lc_wav needs --lc_features mel (the checkpoint names '
                    'no front end)')
        except ValueError as e:
            print(str(e))
            return 1
        args.lc_hop = spec.hop
    elif lpc_on:
        # (--lc_path: the front end the file's frames came from is the
        # checkpoint's)
        try:
            spec = features.spec_from_cli(
                args, wavenet_params['sample_rate'], args.lc_channels, hop,
                stored_lc_features(args.checkpoint, ckpt))
        except ValueError as e:
            print(str(e))
            return 1
    if lpc_on:
        try:
            lp = lpc.from_cli(args, spec, lpc_stored)
        except ValueError as e:
            print(str(e))
            return 1
    if args.lc_wav_dir is not None:
        return _main_dir(args, ckpt, wavenet_params, spec, lc_scales, lc_ctx,
                         emph, lp)
    if args.lc_path is not None or args.lc_wav is not None:
        if args.fast_generation and not args.lc_fast_generation and \
                not args.fast_mixture:
            print('Local conditioning (--lc_path) needs the naive path: '
                  'pass --fast_generation false, or opt in to fast '
                  'generation with local conditioning with '
                  '--lc_fast_generation true.')
            return 1
        from wavenet.audio_reader import upsample_lc
        if args.lc_wav is not None:
            from wavenet.audio_reader import load_wav
            wav = load_wav(args.lc_wav, wavenet_params['sample_rate'])
            if wav.shape[0] == 0:
                print('--lc_wav {} holds no samples'.format(args.lc_wav))
                return 1
            n_wav = min(wav.shape[0], args.samples) if args.samples_given \
                else wav.shape[0]
            feats = spec(wav[:n_wav]).cpu().numpy()
            if lp is not None:
                lp_cf = lp.coefficients_of(wav[:n_wav])
        else:
            feats = np.load(args.lc_path)
            if lp is not None:
                lp_cf = _lpc_from_file(lp, feats, spec)
                if lp_cf is None:
                    print('--lc_path must hold [frames, channels] features '
                          'with the {} mels of the checkpoint\'s front end in '
                          'front'.format(lp.n_mels))
                    return 1
        if feats.ndim != 2 or feats.shape[0] == 0 or args.lc_hop <= 0:
            print('--lc_path must hold [frames, channels] features and '
                  '--lc_hop must be positive')
            return 1
        if lc_scales is not None:
            # (the rows come from the model's upsampler once it is loaded)
            lc_rows = np.zeros((feats.shape[0] * hop, feats.shape[1]),
                               np.float32)
        else:
            lc_rows = upsample_lc(feats, args.lc_hop,
                                  feats.shape[0] * args.lc_hop)
        if n_wav is not None:
            lc_rows = lc_rows[:n_wav]       # (the wav's own length)
        args.samples = lc_rows.shape[0]
    from wavenet import mu_law_decode
    started = "{0:%Y-%m-%dT%H-%M-%S}".format(datetime.now())
    logdir = os.path.join(args.logdir, 'generate', started)
    net = model_from_params(
        wavenet_params, 1, global_condition_channels=args.gc_channels,
        global_condition_cardinality=args.gc_cardinality,
        local_condition_channels=None if lc_rows is None else lc_rows.shape[1],
        local_condition_upsample_scales=lc_scales,
        local_condition_context=lc_ctx, **mol.model_keywords(head))
    why = restore(net, args.checkpoint, args.use_ema, ckpt,
                  check_lc=lc_rows is not None)
    if why:
        print(why)
        return 1
    if lc_scales is not None:
        # the checkpoint's learned upsampler, once for the whole run
        lc_rows = net.upsample_local_condition(
            feats.astype(np.float32), lc_rows.shape[0]).cpu().numpy()
    Q = wavenet_params['quantization_channels']
    rate = wavenet_params['sample_rate']
    gc = None if args.gc_id is None else [args.gc_id]
    if head is not None:
        # float samples on the 16-bit grid (the centres of their levels)
        waveform = _mixture_seed(args, rate, emph)
    elif args.wav_seed:
        waveform = create_seed(args.wav_seed, rate, Q, args.window,
                               emph=emph).cpu().numpy().tolist()
    else:
        waveform = np.random.default_rng(args.seed).integers(
            Q, size=(1,)).tolist()

    # (written in pieces with --save_every: what is filtered is kept with
    # its carry, so the last file is the one written in one go)
    de = None if emph is None else emphasis.DeStream(emph)

    def dump(codes):
        if args.wav_out_path and head is not None:
            out = np.asarray(codes, np.float32)
            if de is not None:
                out = de.feed(out)
            out = _lpc_filter(lp, lp_cf, out, n_seed)
            write_wav16(out, rate, args.wav_out_path)
        elif args.wav_out_path:
            out = mu_law_decode(np.asarray(codes, np.int32), Q).cpu().numpy()
            if de is not None:
                out = de.feed(out)
            out = _lpc_filter(lp, lp_cf, out, n_seed)
            write_wav(out, rate, args.wav_out_path)

    n_seed = len(waveform)
    lc_full = None
    if lc_rows is not None:
        # row of every input position: zeros beside the seed, feature row
        # k beside generated sample k
        n0 = len(waveform)
        lc_full = np.zeros((n0 + args.samples, lc_rows.shape[1]),
                           np.float32)
        lc_full[n0:] = lc_rows

    def rows(pos, n):              # the rows of the n positions from pos
        return None if lc_full is None else lc_full[pos:pos + n]

    if head is not None and args.fast_mixture:
        return _main_mixture(args, net, waveform, rate, logdir, rows, emph,
                             lp, lp_cf)
    if args.clips > 1:
        return _main_clips(args, net, waveform, Q, rate, logdir, rows, emph,
                           lp, lp_cf)
    if head is not None:
        # the naive path: a receptive-field window, predict_mixture, one
        # wn_mol_sample draw per step with counter = step
        net.reserve(1, min(args.window, len(waveform) + args.samples))
        levels = []
        for step in range(args.samples):
            window = waveform[-args.window:]
            lc = None
            if lc_full is not None:
                e = len(waveform)
                lc = lc_full[e - len(window):e][None]
            params = net.predict_mixture(np.asarray(window, np.float32), gc,
                                         local_condition=lc)
            lv, ce = mol.sample(params[None], [args.seed], [step],
                                args.temperature)
            levels.append(int(lv[0]))
            waveform.append(float(ce[0]))
            if (step + 1) % 100 == 0:
                print('Sample {:3<d}/{:3<d}'.format(step + 1, args.samples),
                      end='\r')
            if (args.wav_out_path and args.save_every and
                    (step + 1) % args.save_every == 0):
                dump(waveform)
        print()
        os.makedirs(logdir, exist_ok=True)
        np.save(os.path.join(logdir, 'generated_levels.npy'),
                np.asarray(levels, np.int32))
        dump(waveform)
        print('Finished generating. Levels saved under {}.'.format(logdir))
        return 0
    if args.fast_generation:
        if args.wav_seed:
            print('Priming generation with {} seed samples...'
                  .format(len(waveform)))
        chunk = args.save_every or args.samples
        done = 0
        # first call primes (teacher-forced steps) and starts drawing; later
        # chunks continue from the device-resident queues
        n1 = min(chunk, args.samples)
        codes = net.generate(n1, seed_samples=waveform,
                             temperature=args.temperature,
                             global_condition=gc, seed=args.seed,
                             local_condition=rows(0, len(waveform) + n1 - 1),
                             top_k=args.top_k, top_p=args.top_p)
        waveform = codes.cpu().numpy().tolist()
        done += min(chunk, args.samples)
        if args.save_every and done < args.samples:
            dump(waveform)
        while done < args.samples:
            n = min(chunk, args.samples - done)
            more = net.continue_generation(
                n, waveform[-1], args.temperature, gc, args.seed,
                local_condition=rows(len(waveform) - 1, n),
                top_k=args.top_k, top_p=args.top_p)
            waveform.extend(more.cpu().numpy().tolist())
            done += n
            print('Sample {:3<d}/{:3<d}'.format(done, args.samples), end='\r')
            if args.save_every and done < args.samples:
                dump(waveform)
    else:
        rng = np.random.default_rng(args.seed)
        # one workspace for the whole window: the growing inputs of the first
        # `window` steps are views of it
        net.reserve(1, min(args.window, len(waveform) + args.samples))
        for step in range(args.samples):
            window = waveform[-args.window:] if len(waveform) > args.window \
                else waveform
            lc = None
            if lc_full is not None:
                e = len(waveform)
                lc = lc_full[e - len(window):e][None]
            prediction = net.predict_proba(np.asarray(window), gc,
                                           local_condition=lc
                                           ).cpu().numpy().astype(np.float64)
            # temperature (generate.py:229-233)
            with np.errstate(divide='ignore'):
                scaled = np.log(prediction) / args.temperature
            scaled = np.exp(scaled - np.logaddexp.reduce(scaled))
            if args.temperature == 1.0:
                np.testing.assert_allclose(
                    prediction, scaled, atol=1e-5,
                    err_msg='Prediction scaling at temperature=1.0 is not '
                            'working as intended.')
            if args.top_k is not None or args.top_p is not None:
                # the draw's truncation (wavenet/sampling.py)
                scaled = np.where(sampling.kept_mask(
                    prediction.astype(np.float32), args.temperature,
                    args.top_k, args.top_p), scaled, 0.0)
            waveform.append(int(rng.choice(np.arange(Q), p=scaled / scaled.sum())))
            if (step + 1) % 100 == 0:
                print('Sample {:3<d}/{:3<d}'.format(step + 1, args.samples),
                      end='\r')
            if (args.wav_out_path and args.save_every and
                    (step + 1) % args.save_every == 0):
                dump(waveform)
    print()
    os.makedirs(logdir, exist_ok=True)
    np.save(os.path.join(logdir, 'generated_codes.npy'),
            np.asarray(waveform, np.int32))
    dump(waveform)
    print('Finished generating. Codes saved under {}.'.format(logdir))
    return 0


def _lpc_from_file(lp, feats, spec):
    """The coefficients of --lc_path's frames under the checkpoint's front
    end `spec`: the mel columns (those in front, for a mel+f0 file) with the
    front end's normaliser inverted (lpc.frames_of_file), or None where the
    file does not hold them."""
    raw = lpc.frames_of_file(feats, spec)
    return None if raw is None else lp.coefficients(raw)


def _lpc_filter(lp, cf, out, n_seed):
    """out (numpy float32 [n], the decoded codes: n_seed seed samples, then
    what was generated) with the generated part run through the all-pole
    filter of the frames' coefficients `cf` from a zero state: the whole
    prefix every time, no state is carried between calls.  The seed in front
    stays as decoded."""
    if lp is None or out.shape[0] <= n_seed:
        return out
    out = np.asarray(out, np.float32)
    y = lp.synthesis(out[n_seed:], cf).cpu().numpy()
    return np.concatenate([out[:n_seed], y])


def _main_dir(args, ckpt, wavenet_params, spec, lc_scales, lc_ctx,
              emph=None, lp=None):
    """--lc_wav_dir: copy synthesis of every wav of a directory on --clips
    streams, in length-sorted rounds or through the restart queue
    (--synthesis_schedule; wavenet/synthesis.py)."""
    from wavenet import synthesis
    from wavenet.audio_reader import find_files, load_wav
    rate = wavenet_params['sample_rate']
    files = find_files(args.lc_wav_dir)
    if not files:
        print('--lc_wav_dir {} holds no wav files'.format(args.lc_wav_dir))
        return 1
    audios = [load_wav(f, rate) for f in files]
    if args.samples_given:
        audios = [a[:args.samples] for a in audios]
    for f, a in zip(files, audios):
        if a.shape[0] == 0:
            print('--lc_wav_dir: {} holds no samples'.format(f))
            return 1
    net = model_from_params(
        wavenet_params, 1, global_condition_channels=args.gc_channels,
        global_condition_cardinality=args.gc_cardinality,
        local_condition_channels=spec.channels,
        local_condition_upsample_scales=lc_scales,
        local_condition_context=lc_ctx)
    why = restore(net, args.checkpoint, args.use_ema, ckpt, check_lc=True)
    if why:
        print(why)
        return 1
    try:
        syn, waves = synthesis.copy_synthesize(
            net, spec, audios,
            seeds=[args.seed + i for i in range(len(files))],
            batch=args.clips, global_condition=args.gc_id,
            temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
            schedule=args.synthesis_schedule or 'rounds')
    except ValueError as e:
        print(str(e))
        return 1
    if emph is not None:
        waves = synthesis.deemphasize(emph, waves, syn.rounds)
    if lp is not None:
        waves = synthesis.lpc_synthesize(
            lp, synthesis.lpc_coefficients(lp, audios), waves, syn.rounds)
    synthesis.write_wavs(
        waves, [os.path.splitext(os.path.basename(f))[0] for f in files],
        args.wav_out_dir, rate)
    print('Finished generating {} clips ({} samples in {} lock-step steps, '
          'occupancy {:.3f}) into {}.'.format(
              len(files), sum(a.shape[0] for a in audios), syn.steps,
              syn.occupancy, args.wav_out_dir))
    return 0


def _main_mixture(args, net, waveform, rate, logdir, rows, emph, lp, lp_cf):
    """--fast_mixture true: --clips N streams (default 1) of a mixture-of-
    logistics model in lock step (WaveNetModel.generate_mixture_batch /
    continue_mixture_batch in --save_every chunks), clip i drawing with
    --seed + i, all primed by the same seed.  waveform: the seed as float
    samples on the 16-bit grid."""
    N = args.clips
    seeds = [args.seed + i for i in range(N)]
    gc = args.gc_ids if args.gc_ids is not None else args.gc_id
    seed_lv = mol.levels_reference(np.asarray(waveform, np.float32))[0]
    n_seed = int(seed_lv.shape[0])
    de = None if emph is None else [emphasis.DeStream(emph) for _ in range(N)]

    def dump(levels):
        if args.wav_out_path:
            for i in range(N):
                out = mol.centres(levels[i])
                if de is not None:
                    out = de[i].feed(out)
                out = _lpc_filter(lp, lp_cf, out, n_seed)
                write_wav16(out, rate, args.wav_out_path if N == 1 else
                            _clip_path(args.wav_out_path, i))

    if args.wav_seed:
        print('Priming generation of {} clips with {} seed samples...'
              .format(N, n_seed))
    chunk = args.save_every or args.samples
    done = min(chunk, args.samples)
    parts = [net.generate_mixture_batch(
        done, seeds, seed_lv, args.temperature, gc,
        local_condition=rows(0, n_seed + done - 1)).cpu().numpy()]
    while done < args.samples:
        if args.save_every:
            dump(np.concatenate(parts, axis=1))
        n = min(chunk, args.samples - done)
        parts.append(net.continue_mixture_batch(
            n, parts[-1][:, -1], seeds, args.temperature, gc,
            local_condition=rows(n_seed + done - 1, n)).cpu().numpy())
        done += n
        print('Sample {:3<d}/{:3<d}'.format(done, args.samples), end='\r')
    levels = np.concatenate(parts, axis=1).astype(np.int32)
    print()
    os.makedirs(logdir, exist_ok=True)
    new = levels[:, n_seed:]
    np.save(os.path.join(logdir, 'generated_levels.npy'),
            new[0] if N == 1 else new)
    dump(levels)
    print('Finished generating {} clips. Levels saved under {}.'
          .format(N, logdir))
    return 0


def _clip_path(path, i):
    stem, ext = os.path.splitext(path)
    return '{}_{}{}'.format(stem, i, ext)


def _main_clips(args, net, waveform, Q, rate, logdir, rows=lambda p, n: None,
                emph=None, lp=None, lp_cf=None):
    """--clips N > 1: N streams in lock step (WaveNetModel.generate_batch),
    clip i drawing with --seed + i, all primed by the same seed (and, with
    --lc_path, conditioned on the same rows(position, n))."""
    from wavenet import mu_law_decode
    N = args.clips
    seeds = [args.seed + i for i in range(N)]
    gc = args.gc_ids if args.gc_ids is not None else args.gc_id
    de = None if emph is None else [emphasis.DeStream(emph) for _ in range(N)]

    def dump(codes):
        if args.wav_out_path:
            for i in range(N):
                out = mu_law_decode(np.asarray(codes[i], np.int32), Q
                                    ).cpu().numpy()
                if de is not None:
                    out = de[i].feed(out)
                out = _lpc_filter(lp, lp_cf, out, len(waveform))
                write_wav(out, rate, _clip_path(args.wav_out_path, i))

    if args.wav_seed:
        print('Priming generation of {} clips with {} seed samples...'
              .format(N, len(waveform)))
    chunk = args.save_every or args.samples
    done = min(chunk, args.samples)
    codes = net.generate_batch(done, seeds, seed_samples=waveform,
                               temperature=args.temperature,
                               global_condition=gc,
                               local_condition=rows(0, len(waveform) + done - 1),
                               top_k=args.top_k, top_p=args.top_p
                               ).cpu().numpy()
    parts = [codes]
    while done < args.samples:
        if args.save_every:
            dump(np.concatenate(parts, axis=1))
        n = min(chunk, args.samples - done)
        more = net.continue_generation_batch(
            n, parts[-1][:, -1], seeds, args.temperature, gc,
            local_condition=rows(len(waveform) + done - 1, n),
            top_k=args.top_k, top_p=args.top_p)
        parts.append(more.cpu().numpy())
        done += n
        print('Sample {:3<d}/{:3<d}'.format(done, args.samples), end='\r')
    codes = np.concatenate(parts, axis=1).astype(np.int32)
    print()
    os.makedirs(logdir, exist_ok=True)
    np.save(os.path.join(logdir, 'generated_codes.npy'), codes)
    dump(codes)
    print('Finished generating {} clips. Codes saved under {}.'
          .format(N, logdir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
