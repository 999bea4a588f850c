"""The pieces of train.py's step loop.

Two batch sources with one interface, so that the loop does not ask where a
batch comes from:

    plan(step, B)       host work only: (T, lengths or None, gc or None) of
                        the step's batch.  It may raise (a reader thread that
                        failed); the ranks then agree on the step's fate
                        (parallel.agree_step) before any of them goes on.
    take(step, B, n_t, lengths=None)
                        the planned batch cut to n_t samples: (audio on the
                        device, lc, lc_offset).  lengths: the clips' real
                        lengths as the loss gets them, or None.
    history(step, B, n_t)    the planned batch's leading history samples per
                        clip, cut to n_t (host int64 [B]), or None for a
                        source without history (train.py --piece_history)
    start(device) / stop()   the reader threads; device: the model's.
    checkpoint_entry(step), gc_category_cardinality, lc

`lc` says what the source's local conditioning is: 'frames' (frame-rate
features and each clip's offset, for a model with a learned upsampler),
'rows' (one row per sample) or None -- none at all, or computed in take by
`front` (a callable (audio [B, T], lengths) -> lc the loop sets: --lc_features
mel with piece context) from the batch as cut.

Pre-emphasis (`emphasis`: an emphasis.Emphasis or None, train.py
--preemphasis): take pre-emphasises the batch's audio AFTER the features have
been computed from the raw batch -- the model sees the emphasised signal, the
features are those of the natural one.  The filter is of the piece: a piece's
first sample sees a zero in front of it, as its mel frames see zeros.  The
output goes into a buffer of the source's own, two used in turn; the batch
itself (a view of the corpus's ring) is not rewritten.

Linear prediction (`lpc`: an lpc.LinearPrediction or None, train.py
--lpc_order) takes the same place: take computes the raw log-mel of the batch
as cut (a launch of its own beside the front end's), the predictor
coefficients of every frame and then the excitation into one of the two
buffers.  The model sees the excitation, the features are those of the
natural signal.

StepLog prints and logs the loss lines, one step late; validate scores the
held-out set.
"""
from __future__ import print_function

import contextlib
import json
import os
import time

import numpy as np
import torch

from . import parallel


class StageIn(object):
    """host [B, n] float tensor -> device tensor, copied on a stream of its
    own: the (pageable, hence host-blocking) copy then does not queue behind
    the previous step's kernels, and the training stream only waits for the
    copy.  (Pinned staging buffers measured 33 instead of 9.6 ms per step on
    this platform, tools/h2d_probe.py.)"""

    def __init__(self, device):
        self.device, self.stream = device, None

    def __call__(self, host):
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self.stream):
            dev = host.contiguous().to(self.device)
        torch.cuda.current_stream().wait_stream(self.stream)
        dev.record_stream(torch.cuda.current_stream())
        return dev


class _ShapedSource(object):
    """What the two sources share: `front` and the shaping filter of a batch
    (pre-emphasis, or the linear-prediction excitation) into one of two
    buffers of the source's own."""
    front = None
    lpc = None

    def history(self, step, B, n_t):
        return None

    def _buffer(self, audio):
        """One of the source's two buffers, used in turn, as a tensor of
        audio's shape."""
        if not hasattr(self, '_shape_bufs'):
            self._shape_bufs, self._shape_calls = [None, None], 0
        slot = self._shape_calls & 1
        self._shape_calls += 1
        buf = self._shape_bufs[slot]
        if buf is None or buf.numel() < audio.numel() or \
                buf.device != audio.device:
            buf = self._shape_bufs[slot] = torch.empty(
                audio.numel(), dtype=torch.float32, device=audio.device)
        return buf[:audio.numel()].view(audio.shape)

    def _shape(self, audio, lengths):
        """audio: device float32 [B, T], left as it is: its pre-emphasis, or
        its linear-prediction excitation."""
        if self.lpc is not None:
            cf = self.lpc.coefficients_of(audio, lengths)
            return self.lpc.analysis(audio, cf, lengths,
                                     out=self._buffer(audio))
        if self.emphasis is None:
            return audio
        return self.emphasis.pre(audio, lengths, out=self._buffer(audio))

    def _finish(self, audio, lc, lengths):
        """(audio, lc) with `front`'s features of the raw batch where the
        loop set one, then the shaping filter."""
        if self.front is not None:
            lc = self.front(audio.reshape(audio.shape[0], -1), lengths)
        if self.emphasis is not None or self.lpc is not None:
            audio = self._shape(audio.reshape(audio.shape[0], -1), lengths)
        return audio, lc


class ReaderSource(_ShapedSource):
    """Batches of an AudioReader or a SyntheticReader: plan dequeues the host
    batch and holds it, take cuts it and copies the audio to the device."""

    def __init__(self, reader, coord, lengths=False, gc=False, lc=None,
                 emphasis=None):
        self.reader, self.coord = reader, coord
        self.lengths, self.gc, self.lc = lengths, gc, lc
        self.emphasis = emphasis
        self.gc_category_cardinality = reader.gc_category_cardinality
        self.threads, self.held = [], None

    def start(self, device):
        self.device, self.stage_in = device, StageIn(device)
        self.threads = self.reader.start_threads()

    def stop(self):
        self.coord.request_stop()
        self.coord.join(self.threads)

    def plan(self, step, B):
        # (this order: the readers pair lengths, ids and features with "the
        # last dequeue")
        reader, lc, lc_off = self.reader, None, 0
        audio = reader.dequeue(B)
        lengths = reader.dequeue_lengths(B).numpy() if self.lengths else None
        gc = reader.dequeue_gc(B) if self.gc else None
        if self.lc == 'frames':
            # frames + offsets: the model upsamples on the device
            lc, lc_off = reader.dequeue_lc_frames(B)
        elif self.lc == 'rows':
            lc = reader.dequeue_lc(B)
        self.held = audio, lc, lc_off
        return audio.shape[1], lengths, gc

    def take(self, step, B, n_t, lengths=None):
        audio, lc, lc_off = self.held
        audio = audio[:, :n_t]
        if self.lc == 'rows':
            lc = lc[:, :n_t]
        if audio.device.type == 'cpu' and self.device.type == 'cuda':
            # a pageable copy on a side stream (StageIn): handed to net.loss
            # as it is, the host tensor would be copied synchronously BEHIND
            # the previous step's kernels, i.e. the host would wait for the
            # device every step and prepare the next batch while it idles
            audio = self.stage_in(audio.reshape(audio.shape[0], -1))
        audio, lc = self._finish(audio, lc, lengths)
        return audio, lc, lc_off

    def checkpoint_entry(self, step):
        return None


class CorpusSource(_ShapedSource):
    """Batches of a corpus.DeviceCorpus: plan reads the host index alone, take
    cuts the batch on the device (one or two launches on the training stream,
    no copy).  Step k takes batch `base` + k; `entry`: the corpus's settings
    as checkpoints store them under 'device_corpus'."""

    def __init__(self, corpus, entry, lengths=False, gc=False, lc=None,
                 emphasis=None):
        self.corpus, self.entry, self.base = corpus, entry, 0
        self.lengths, self.gc, self.lc = lengths, gc, lc
        self.emphasis = emphasis
        self.gc_category_cardinality = corpus.gc_category_cardinality

    def start(self, device):
        pass

    def stop(self):
        pass

    def plan(self, step, B):
        # (with history the loss always gets the lengths: a slot's history
        # is counted from its own first sample)
        p = self.corpus.plan(self.base + step, B)
        with_n = self.lengths or self.corpus.index.history > 0
        return (p.T, p.n if with_n else None,
                torch.from_numpy(p.gc) if self.gc else None)

    def history(self, step, B, n_t):
        if not self.corpus.index.history:
            return None
        return self.corpus.plan(self.base + step, B, T=n_t).history

    def take(self, step, B, n_t, lengths=None):
        cb = self.corpus.batch(self.base + step, B, T=n_t, lc=self.lc)
        # (the front end gets the lengths the loss gets; the filter the
        # batch's own: its padding is zeros either way)
        audio, lc = cb.audio, cb.frames if self.lc == 'frames' else cb.rows
        if self.front is not None:
            lc = self.front(audio, lengths)
        # (an empty slot is all zeros: one sample of it gives the same)
        audio = self._shape(audio, np.maximum(cb.lengths, 1))
        return audio, lc, cb.offsets if self.lc == 'frames' else 0

    def checkpoint_entry(self, step):
        """The 'device_corpus' entry of a checkpoint after step `step`."""
        return dict(self.entry, batch=self.base + step)


class _Done(object):
    def synchronize(self):
        pass


class StepLog(object):
    """The training lines and <logdir>/events.jsonl (rank 0 writes).

    The reference fetches the loss inside sess.run and so waits for every
    step (train.py:300-311).  Here a step is queued on the device and its loss
    is read ONE step later, while the next step runs (the same lines, one step
    late; 12.0 -> 9.5 ms per step at 8 x 16000: bench.py's step time): step()
    reports the step before and holds its own until the next call or flush().
    Call flush() where a step's own state is needed at once: a checkpoint
    step, a traced step, the last step."""

    def __init__(self, net, logdir, rank):
        self.net, self.rank = net, rank
        self.events = None
        if rank == 0:
            os.makedirs(logdir, exist_ok=True)
            self.events = open(os.path.join(logdir, 'events.jsonl'), 'a')
        self.pending = None         # the step not yet printed
        self.last_report = None
        self.slots, self.issued = {}, {}

    def fetch_later(self, t, tag=0):
        """(pinned host scalar, event): the scalar holds t once the event has
        completed.  Two slots per `tag`, taken in turn by the fetches issued:
        a fetch is read before the one after next is issued, whatever the
        steps' numbers are."""
        if not t.is_cuda:
            return t.detach().reshape(()).clone(), _Done()
        n = self.issued.get(tag, 0)
        self.issued[tag] = n + 1
        key = 2 * tag + (n & 1)
        if key not in self.slots:
            self.slots[key] = (torch.empty((), dtype=torch.float32)
                               .pin_memory(), torch.cuda.Event())
        host_scalar, done = self.slots[key]
        host_scalar.copy_(t.detach().reshape(()).float(), non_blocking=True)
        done.record()
        return host_scalar, done

    def step(self, k, loss, norm, started, real=None):
        """Step k is queued: average its loss over the ranks, start the fetch
        of it and of `norm` (--clip_norm: the norm before clipping, or None),
        and report the step before.  `real`: --mask_padding's real samples."""
        # (the norm first: the loss's event, recorded behind both copies,
        # then covers it.  Every rank holds the same norm: no collective)
        norm = None if norm is None else self.fetch_later(norm, tag=1)
        mean_loss = self.fetch_later(parallel.allreduce_mean_scalar(loss))
        self.flush()
        self.pending = (k, mean_loss, started, real, norm)

    def flush(self):
        if self.pending is not None:
            self._report(*self.pending)
            self.pending = None

    def _report(self, k, mean_loss, started, real, norm):
        """Fetch step k's loss (waits for that step), check it, print / log the
        reference's line (train.py:310-311).  sec/step: from the previous line
        (the pipeline's cadence), or from the step's start for the first."""
        # (float(tensor) would wait for EVERYTHING queued on the stream, the
        # next step included: the loss went to a pinned scalar behind an event)
        host_scalar, done = mean_loss
        done.synchronize()
        loss_value = float(host_scalar)
        # (the norm was copied behind the loss on the same stream: complete
        # once the loss's event is)
        norm_value = None if norm is None else float(norm[0])
        if not np.isfinite(loss_value):
            # every rank sees the same NaN mean: decide TOGETHER whether a
            # kernel reported an error, so that no rank is left waiting in
            # the next step's collectives
            dev_err = None
            try:
                self.net.check_device_errors()
            except Exception as e:
                dev_err = e
            if parallel.any_rank(dev_err is not None, self.net.device):
                raise dev_err or RuntimeError(
                    'rank %d: another rank reported an expired dependency '
                    'wait in a persistent stack launch at step %d'
                    % (self.rank, k))
        now = time.time()
        duration = now - (self.last_report if self.last_report is not None
                          and self.last_report > started else started)
        self.last_report = now
        if self.rank == 0:
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
            self._write(line)

    def validation(self, k, res):
        """The validation line after step k (res: evaluate.summary's)."""
        if self.rank == 0:
            # (a mixture-of-logistics head reports no accuracy)
            print('step {:d} - validation loss = {:.3f}, bits/sample = {:.3f}'
                  .format(k, res['nll_per_sample'], res['bits_per_sample']) +
                  ('' if res['accuracy'] is None else
                   ', accuracy = {:.3f}'.format(res['accuracy'])))
            self._write({
                'step': k, 'validation_loss': res['nll_per_sample'],
                'validation_bits': res['bits_per_sample'],
                'validation_accuracy': res['accuracy'],
                'validation_samples': res['samples']})

    def _write(self, line):
        self.events.write(json.dumps(line) + '\n')
        self.events.flush()

    def close(self):
        if self.events:
            self.events.close()


def validate(net, optimizer, vset, spec, args, emphasis=None, lpc=None):
    """Score the validation set with the weights as they are (the EMA shadow
    with --validate_ema): every rank its shard, ONE sum over the ranks
    whatever a shard holds (a set built with history: each piece behind its
    left context, which is not scored); with `emphasis` the audio is pre-emphasised
    behind the front end, as the training batches are (with `lpc` it is
    replaced by its excitation).  Returns
    evaluate.summary's dict."""
    from . import evaluate as ev
    swap = ev.parameters_swapped(net, optimizer.ema_flat(net)) \
        if args.validate_ema else contextlib.nullcontext()
    with swap:
        batches = vset.batches(args.batch_size)
        if spec is not None:
            batches = ev.with_features(net, spec, batches)
        if emphasis is not None:
            batches = ev.with_emphasis(emphasis, batches)
        if lpc is not None:
            batches = ev.with_lpc(lpc, spec, batches)
        tot = ev.totals(net, batches, args.validation_batches)
    return ev.summary(ev.sum_over_ranks(tot, net.device))
