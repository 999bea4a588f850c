"""Everything that reads or writes a `model.ckpt-<step>`.

train.py writes torch files holding {'variables': {reference variable name:
tensor}, 'step'} and, where the run has them, 'optimizer', 'ema_variables',
'lc_features', 'device_corpus', 'emphasis', 'input_noise', 'lpc' and
'output'; the step is parsed from the file name, as
in the reference (train.py:104-134 there).  The reference's own TensorFlow
checkpoints are read too (tf_checkpoint.py).  train.py, generate.py and
evaluate.py import their checkpoint functions from here.
"""
from __future__ import print_function

import collections
import glob
import os
import re
import sys

import numpy as np
import torch

from . import tf_checkpoint

# open_latest's result.  ckpt: the torch dict, or None for a checkpoint that
# tf.train.Saver wrote (tf_checkpoint reads those variable by variable)
Opened = collections.namedtuple('Opened', 'path step ckpt')
_NOT_OPENED = object()


def checkpoint_path(logdir, step):
    return os.path.join(logdir, 'model.ckpt-{}'.format(step))


def save(net, logdir, step, optimizer=None, lc_features=None,
         device_corpus=None, emphasis=None, input_noise=None, lpc=None,
         output=None):
    """`optimizer`: its step count, slots and shadow go in as 'optimizer'
    and, with EMA weights, the shadow as 'ema_variables' (the keys of
    'variables').  `lc_features`: the front end's settings
    (features.checkpoint_entry), stored under 'lc_features'.
    `device_corpus`: the settings of --device_corpus (crop, seed,
    sample_size, lc_feature_context) and the index of the last batch taken
    ('batch'), stored under 'device_corpus'.  `emphasis`: the pre-emphasis
    the model was trained on (emphasis.Emphasis.entry: {'alpha': ..}),
    stored under 'emphasis'; a run without it writes no such entry.
    `input_noise`: the noise the run's inputs were perturbed with
    (input_noise.InputNoise.entry: {'prob', 'width', 'seed'}), stored under
    'input_noise', likewise only where given.  `lpc`: the linear prediction
    whose excitation the model was trained on (lpc.LinearPrediction.entry:
    {'order', 'noise', 'lag_window', 'gain'}), stored under 'lpc', likewise.
    `output`: the head of a model that does not end in the softmax
    (mol.output_entry: {'kind': 'mol', 'components', 'log_scale_min',
    'levels'}), stored under 'output', likewise."""
    print('Storing checkpoint to {} ...'.format(logdir), end="")
    sys.stdout.flush()
    os.makedirs(logdir, exist_ok=True)
    path = checkpoint_path(logdir, step)
    ckpt = {'variables': net.state_dict(), 'step': step}
    if lc_features is not None:
        ckpt['lc_features'] = lc_features
    if device_corpus is not None:
        ckpt['device_corpus'] = device_corpus
    if emphasis is not None:
        ckpt['emphasis'] = emphasis
    if input_noise is not None:
        ckpt['input_noise'] = input_noise
    if lpc is not None:
        ckpt['lpc'] = lpc
    if output is not None:
        ckpt['output'] = output
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


def open_latest(logdir):
    """Find and read logdir's newest checkpoint, printing nothing:
    Opened(path, step, the torch dict -- None for one of the reference's),
    or None where the directory holds no checkpoint."""
    path = latest_checkpoint(logdir) if os.path.isdir(logdir) else None
    if path is None:
        return None
    step = int(path.split('/')[-1].split('-')[-1])
    if tf_checkpoint.checkpoint_format(path):
        return Opened(path, step, None)
    return Opened(path, step, torch.load(path, map_location='cpu'))


def load(net, logdir, optimizer=None, entries=None, opened=_NOT_OPENED):
    """`optimizer`: restored from the checkpoint's 'optimizer' entry when it
    has one (checkpoints written before it existed, and the reference's own,
    have none: the optimizer then starts afresh, as it always did).
    `entries`: a dict that receives the checkpoint's 'device_corpus' entry.
    `opened`: open_latest(logdir)'s result where the caller holds it."""
    print("Trying to restore saved checkpoints from {} ...".format(logdir),
          end="")
    if opened is _NOT_OPENED:
        opened = open_latest(logdir)
    if opened is None:
        print(" No checkpoint found.")
        return None
    path, global_step, ckpt = opened
    print("  Checkpoint found: {}".format(path))
    print("  Global step was: {}".format(global_step))
    print("  Restoring...", end="")
    if ckpt is None:
        # written by the reference's tf.train.Saver (train.py:104-114 there)
        tf_checkpoint.load_into(net, path)
    else:
        net.load_state_dict(ckpt['variables'])
        if optimizer is not None and 'optimizer' in ckpt:
            optimizer.load_state_dict(ckpt['optimizer'], net)
        if entries is not None and 'device_corpus' in ckpt:
            entries['device_corpus'] = ckpt['device_corpus']
    print(" Done.")
    return global_step


def upsampler_mismatch(net, sd):
    """A message when the checkpoint's upsampler variables (state dict `sd`)
    and the model's (--lc_upsample_scales) differ, else None."""
    mine = {n: tuple(v.shape) for n, v in net.named_variables()
            if '/lc_upsample/' in n}
    theirs = {n: tuple(np.shape(v)) for n, v in sd.items()
              if '/lc_upsample/' in n}
    if mine == theirs:
        return None
    def desc(d):
        filt = [d[n][0] for n in sorted(d) if n.endswith('/filter')]
        return ','.join(str(s) for s in filt) if filt else 'none'
    return ('the checkpoint\'s learned upsampler (wavenet/lc_upsample/..., '
            'scales %s) does not match --lc_upsample_scales (scales %s)'
            % (desc(theirs), desc(mine)))


def context_mismatch(net, sd):
    """A message when the checkpoint's frame-context filter (state dict
    `sd`) and the model's (--lc_context) differ, else None."""
    name = 'wavenet/lc_context/filter'
    mine = dict(net.named_variables()).get(name)
    mine = None if mine is None else tuple(mine.shape)
    theirs = tuple(np.shape(sd[name])) if name in sd else None
    if mine == theirs:
        return None
    def desc(shape):
        return 'none' if shape is None else 'P = %d, shape %s' % (
            (shape[0] - 1) // 2, 'x'.join(str(n) for n in shape))
    return ('the checkpoint\'s frame-context filter (%s, %s) does not match '
            '--lc_context (%s)' % (name, desc(theirs), desc(mine)))


def open_ema_checkpoint(path):
    """--use_ema true: (the checkpoint, None), or (None, why it holds no EMA
    weights)."""
    if tf_checkpoint.checkpoint_format(path):
        return None, ('--use_ema true: a TensorFlow checkpoint holds no EMA '
                      'weights.')
    ckpt = torch.load(path, map_location='cpu')
    if 'ema_variables' not in ckpt:
        return None, ('--use_ema true: the checkpoint {} holds no EMA weights '
                      '(`ema_variables`); train with train.py --ema_decay.'
                      .format(path))
    return ckpt, None


def stored_lc_features(path, ckpt=None):
    """The 'lc_features' entry train.py --lc_features wrote into the
    checkpoint at `path` (`ckpt` where the caller holds it), else None."""
    if ckpt is None:
        if tf_checkpoint.checkpoint_format(path) or not os.path.isfile(path):
            return None
        ckpt = torch.load(path, map_location='cpu')
    return ckpt.get('lc_features')


def stored_emphasis(path, ckpt=None):
    """The 'emphasis' entry train.py --preemphasis wrote into the checkpoint
    at `path` (`ckpt` where the caller holds it), else None."""
    if ckpt is None:
        if tf_checkpoint.checkpoint_format(path) or not os.path.isfile(path):
            return None
        ckpt = torch.load(path, map_location='cpu')
    return ckpt.get('emphasis')


def stored_lpc(path, ckpt=None):
    """The 'lpc' entry train.py --lpc_order wrote into the checkpoint at
    `path` (`ckpt` where the caller holds it), else None."""
    if ckpt is None:
        if tf_checkpoint.checkpoint_format(path) or not os.path.isfile(path):
            return None
        ckpt = torch.load(path, map_location='cpu')
    return ckpt.get('lpc')


def stored_output(path, ckpt=None):
    """The 'output' entry train.py --output_mixture wrote into the
    checkpoint at `path` (`ckpt` where the caller holds it), else None."""
    if ckpt is None:
        if tf_checkpoint.checkpoint_format(path) or not os.path.isfile(path):
            return None
        ckpt = torch.load(path, map_location='cpu')
    return ckpt.get('output')


def restore(net, path, use_ema=False, ckpt=None, check_lc=False):
    """Load the checkpoint at `path` into `net` (generate.py and evaluate.py):
    the reference's own TensorFlow format, or train.py's torch file `ckpt`
    (read here unless the caller holds it), its `ema_variables` with use_ema.
    check_lc: compare the learned upsampler's and the context filter's shapes
    first.  Returns a message when they do not match, else None."""
    print('Restoring model from {}'.format(path))
    if tf_checkpoint.checkpoint_format(path):
        # a checkpoint written by the reference itself (tf.train.Saver)
        tf_checkpoint.load_into(net, path)
        return None
    if ckpt is None:
        ckpt = torch.load(path, map_location='cpu')
    sd = ckpt['ema_variables' if use_ema else 'variables']
    if check_lc:
        why = upsampler_mismatch(net, sd) or context_mismatch(net, sd)
        if why:
            return why
    net.load_state_dict(sd)
    return None
