"""Listen to a feature file without a trained model: Griffin-Lim on the device
(wavenet/griffin_lim.py) from log-mel frames, or from a wav through the front
end and back.  No network runs.

    python tools/griffin_lim.py IN.npy --out OUT.wav --checkpoint CKPT
    python tools/griffin_lim.py IN.wav --out OUT.wav --sample_rate 16000 \\
        --lc_channels 80 --lc_hop 256 [--lc_n_fft 1024 --lc_win_length 1024
        --lc_fmin 0 --lc_fmax 8000] [--gl_iterations 32 --gl_momentum 0.99
        --seed 0]

The front end's settings come from --checkpoint (its 'lc_features' entry, what
train.py --lc_features stored) or from the flags tools/make_lc_features.py
takes; flags beside a checkpoint replace single settings.

IN.npy holds frames [F, channels] as tools/make_lc_features.py writes them:
where the front end has a normaliser it is inverted first (Normalizer.invert:
clamped values do not come back), the F0 and voicing channels of a mel+f0
front end are dropped, and OUT.wav has F * hop samples.  Every frame is taken
as it stands: the zero frames make_lc_features.py writes outside the
utterance are log-power 0, not silence.  IN.wav is loaded at the front end's
sample rate, its raw log-mel features are computed on the device and inverted:
OUT.wav has the input's length and is what evaluate.py --synthesis_baseline
griffin_lim compares a model against.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
from wavenet import features  # noqa: E402

GL_ITERATIONS, GL_MOMENTUM = 32, 0.99


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('input', metavar='IN.{npy,wav}')
    p.add_argument('--out', type=str, required=True, help='the wav to write')
    p.add_argument('--checkpoint', type=str, default=None,
                   help='take the front end from this checkpoint\'s '
                   '\'lc_features\' entry')
    p.add_argument('--sample_rate', type=int, default=None)
    p.add_argument('--lc_channels', type=int, default=None,
                   help='the number of mels (--lc_features mel+f0: two more)')
    p.add_argument('--lc_hop', type=int, default=None,
                   help='audio samples per feature frame')
    p.add_argument('--gl_iterations', type=int, default=GL_ITERATIONS,
                   help='Griffin-Lim iterations in [0, 4096] (default %d)'
                   % GL_ITERATIONS)
    p.add_argument('--gl_momentum', type=float, default=GL_MOMENTUM,
                   help='Fast Griffin-Lim momentum in [0, 1) (default %g)'
                   % GL_MOMENTUM)
    p.add_argument('--seed', type=int, default=0,
                   help='seed of the starting phases (default 0)')
    features.add_cli_flags(p, '  (Implied here.)')
    a = p.parse_args(argv)
    if os.path.splitext(a.input)[1].lower() not in ('.npy', '.wav'):
        p.error('IN must be an .npy of frames or a .wav, got %r' % a.input)
    if a.lc_features == 'none':
        p.error('--lc_features none: nothing to invert')
    if a.checkpoint is None:
        for name in ('sample_rate', 'lc_channels', 'lc_hop'):
            if getattr(a, name) is None:
                p.error('--%s is required without --checkpoint' % name)
        a.lc_features = a.lc_features or 'mel'
    if not 0 <= a.gl_iterations <= 4096:
        p.error('--gl_iterations must be in [0, 4096], got %d'
                % a.gl_iterations)
    if not 0 <= a.gl_momentum < 1:
        p.error('--gl_momentum must be in [0, 1), got %r' % a.gl_momentum)
    if a.seed < 0:
        p.error('--seed must not be negative, got %d' % a.seed)
    if features.f0_flags_refused(a, stored_may_decide=a.checkpoint is not None):
        p.error(features.f0_flags_refused(
            a, stored_may_decide=a.checkpoint is not None))
    return a


def front_end(args):
    """The spec of the flags and the checkpoint (ValueError where they do not
    fit or name none)."""
    stored = None
    if args.checkpoint is not None:
        from wavenet.checkpoint import stored_lc_features
        stored = stored_lc_features(args.checkpoint)
        if stored is None and args.lc_features is None:
            raise ValueError("%s names no front end (no 'lc_features' entry)"
                             % args.checkpoint)
    rate = args.sample_rate
    if rate is None and stored is not None:
        rate = stored.get('sample_rate')
    if rate is None:
        raise ValueError('--sample_rate is required: the checkpoint names none')
    spec = features.spec_from_cli(args, rate, args.lc_channels, args.lc_hop,
                                  stored)
    if spec is None:
        raise ValueError('no front end: give --lc_features mel')
    return spec


def frames_of(spec, path):
    """(raw log-mel frames float32 [F, n_mels], samples or None) of IN."""
    mel = spec if isinstance(spec, features.MelSpec) else spec.mel
    raw = mel.with_normalizer(None)
    if path.lower().endswith('.wav'):
        from wavenet import audio_reader as ar
        audio = np.asarray(ar.load_wav(path, int(mel.sample_rate)),
                           np.float32).reshape(-1)
        if audio.shape[0] < 1:
            raise ValueError('%s holds no samples' % path)
        return raw(audio), int(audio.shape[0])
    frames = np.load(path)
    if frames.ndim != 2 or frames.shape[0] < 1 or \
            frames.shape[1] != spec.channels:
        raise ValueError('%s: frames [F, %d] are required, got %s'
                         % (path, spec.channels, list(frames.shape)))
    frames = np.ascontiguousarray(frames[:, :mel.n_mels], np.float32)
    # (the spec's own normaliser: a MelPitchSpec's .mel never carries one)
    if spec.normalizer is not None:
        frames = spec.normalizer.invert(frames)
    return frames, None


def main(argv=None):
    args = get_arguments(argv)
    from wavenet import griffin_lim
    try:
        spec = front_end(args)
        mel = spec if isinstance(spec, features.MelSpec) else spec.mel
        gl = griffin_lim.GriffinLim(
            mel.with_normalizer(None), iterations=args.gl_iterations,
            momentum=args.gl_momentum, seed=args.seed)
        frames, n = frames_of(spec, args.input)
        wave = gl(frames, lengths=None if n is None else [n])
    except (ValueError, OSError) as e:
        print(str(e))
        return 1
    from scipy.io import wavfile
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    wavfile.write(args.out, int(mel.sample_rate),
                  wave.detach().cpu().numpy().astype(np.float32))
    print('%s: %d samples from %d frames' % (args.out, int(wave.shape[0]),
                                             int(frames.shape[0])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
