"""Per-channel statistics of the log-mel features of every wav under DIR, for
train.py / evaluate.py / generate.py --lc_normalize corpus --lc_stats FILE:
the pass train.py --device_corpus true --lc_normalize corpus makes at load
(wavenet/corpus.py), on its own.

    python tools/make_lc_stats.py DIR --sample_rate 16000 --lc_channels 80 \\
        --lc_hop 256 --out stats.npz [--silence_threshold 0.3]
        [--lc_n_fft 1024 --lc_win_length 1024 --lc_fmin 0 --lc_fmax 8000]

Every file is loaded and trimmed by AudioReader's own functions, its
utterance's frames are computed on the device and their sums of x and x * x
accumulated in float64 in one fixed order (features.FeatureStats).  The .npz
holds `count` (frames), `s1` and `s2` [lc_channels].  Give
--silence_threshold as to train.py (its default is train.py's).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

from wavenet import features  # noqa: E402

SILENCE_THRESHOLD = 0.3        # train.py's


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('directory', metavar='DIR',
                   help='searched recursively for *.wav')
    p.add_argument('--sample_rate', type=int, required=True,
                   help='the model\'s sample rate (wavenet_params.json)')
    p.add_argument('--lc_channels', type=int, required=True,
                   help='the number of mels (--lc_features mel+f0: the '
                   'model\'s channels, two more than the mels; the '
                   'statistics are those of the mels)')
    p.add_argument('--lc_hop', type=int, required=True,
                   help='audio samples per feature frame')
    p.add_argument('--silence_threshold', type=float,
                   default=SILENCE_THRESHOLD)
    p.add_argument('--out', type=str, required=True,
                   help='the .npz to write')
    features.add_cli_flags(p, '  (Implied here.)')
    args = p.parse_args(argv)
    if args.lc_features == 'none':
        p.error('--lc_features none: nothing to measure')
    for flag in ('lc_normalize', 'lc_norm_clip', 'lc_range', 'lc_stats'):
        if getattr(args, flag) is not None:
            p.error('--%s: the statistics are those of the raw features'
                    % flag)
    args.lc_features = args.lc_features or 'mel'
    if features.f0_flags_refused(args):
        p.error(features.f0_flags_refused(args))
    return args


def main(argv=None):
    args = get_arguments(argv)
    from wavenet.corpus import DeviceCorpus
    try:
        spec = features.spec_from_cli(args, args.sample_rate,
                                      args.lc_channels, args.lc_hop)
        # (the frames are summed utterance by utterance, none are kept)
        corpus = DeviceCorpus(args.directory, args.sample_rate, False,
                              silence_threshold=args.silence_threshold)
    except (ValueError, MemoryError) as e:
        print(str(e))
        return 1
    stats = corpus.compute_feature_stats(spec)
    stats.save(args.out)
    mean, std = stats.mean(), stats.std()
    print('{}: {} frames of {} files, mean {:.3f} .. {:.3f}, std {:.3f} .. '
          '{:.3f}'.format(args.out, stats.count, len(corpus.files),
                          mean.min(), mean.max(), std.min(), std.max()))
    return 0


if __name__ == '__main__':
    sys.exit(main())
