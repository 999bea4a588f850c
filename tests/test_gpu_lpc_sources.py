"""The training sources' shaping step (wavenet/training.py): the pre-emphasis
or the linear-prediction excitation of a batch goes into one of TWO buffers of
the source's own, used in turn -- the third take reuses the first's memory, the
second's stays intact meanwhile -- and a DeviceCorpus batch is never
rewritten."""
import numpy as np
import pytest
import torch

import lpc_ref as R

pytestmark = pytest.mark.gpu

B, T = 3, 400


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def corpus(hip_lib, tmp_path_factory):
    from scipy.io import wavfile
    from wavenet.corpus import DeviceCorpus
    tmp = tmp_path_factory.mktemp('lpc_sources')
    rng = np.random.default_rng(8)
    for i in range(5):
        m = 1100 + 211 * i
        x = 0.6 * np.sin(2 * np.pi * 220.0 * (i + 1) * np.arange(m) / 16000.0) \
            + 0.05 * rng.standard_normal(m)
        wavfile.write(str(tmp / ('c%d.wav' % i)), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    return DeviceCorpus(str(tmp), 16000, False, sample_size=500,
                        silence_threshold=None)


def _filters():
    from wavenet.emphasis import Emphasis
    lp = R.make_lp(8, 8, 64, 16, gain=2.0)
    return {'emphasis': dict(emphasis=Emphasis(0.97)), 'lpc': dict(lpc=lp)}


def _want(kind, kw, audio, lengths):
    """The filter's own result on the raw batch, as bytes."""
    if kind == 'emphasis':
        return kw['emphasis'].reference_pre(audio.cpu().numpy(),
                                            lengths).tobytes()
    lp = kw['lpc']
    return _bits(lp.analysis(audio, lp.coefficients_of(audio, lengths),
                             lengths))


def _three_takes(take, raw, kind, kw):
    """take(k) -> shaped audio of batch k; raw(k) -> (audio, lengths)."""
    outs = [take(k) for k in range(3)]
    for o in outs:
        assert o.shape == (B, T) and o.dtype == torch.float32
    p = [o.data_ptr() for o in outs]
    # two buffers, used in turn
    assert p[2] == p[0] and p[1] != p[0]
    lo, hi = sorted(p[:2])
    assert lo + 4 * B * T <= hi
    # the second take's result outlives the third take; the third holds its own
    for k in (1, 2):
        assert _bits(outs[k]) == _want(kind, kw, *raw(k)), (kind, k)
    # a fourth take goes into the second buffer
    assert take(3).data_ptr() == p[1]


@pytest.mark.parametrize('kind', ['emphasis', 'lpc'])
def test_corpus_source_uses_two_buffers_in_turn(corpus, kind):
    from wavenet import training
    kw = _filters()[kind]
    src = training.CorpusSource(corpus, {}, lengths=True,
                                emphasis=kw.get('emphasis'))
    src.lpc = kw.get('lpc')
    raws = {}

    def raw(k):
        if k not in raws:
            cb = corpus.batch(k, B, T=T)
            raws[k] = (cb.audio.clone(), np.maximum(cb.lengths, 1))
        return raws[k]
    for k in range(4):
        raw(k)

    def take(k):
        src.plan(k, B)
        out = src.take(k, B, T)[0]
        # the corpus's own batch is not rewritten, and is not the output
        again = corpus.batch(k, B, T=T)
        assert _bits(again.audio) == _bits(raws[k][0])
        assert out.data_ptr() != again.audio.data_ptr()
        return out
    _three_takes(take, raw, kind, kw)


class _Reader(object):
    """The least a ReaderSource asks of a reader: host batches [B, T, 1]."""
    gc_category_cardinality = None

    def __init__(self):
        rng = np.random.default_rng(4)
        self.batches = [torch.from_numpy(
            rng.uniform(-0.5, 0.5, (B, T, 1)).astype(np.float32))
            for _ in range(4)]
        self.k = -1

    def dequeue(self, n):
        self.k += 1
        return self.batches[self.k]

    def dequeue_lengths(self, n):
        return torch.tensor([T, T - 37, 90])


@pytest.mark.parametrize('kind', ['emphasis', 'lpc'])
def test_reader_source_uses_two_buffers_in_turn(hip_lib, kind):
    from wavenet import training
    kw = _filters()[kind]
    reader = _Reader()
    src = training.ReaderSource(reader, None, lengths=True,
                                emphasis=kw.get('emphasis'))
    src.lpc = kw.get('lpc')
    src.device = torch.device('cuda', torch.cuda.current_device())
    src.stage_in = training.StageIn(src.device)
    n = np.array([T, T - 37, 90])

    def raw(k):
        return reader.batches[k].reshape(B, T).to(src.device), n

    def take(k):
        _, lengths, _ = src.plan(k, B)
        return src.take(k, B, T, lengths)[0]
    _three_takes(take, raw, kind, kw)
