"""Guard bands around kernel operands: the only way this suite can see a
launch that reads or writes outside the memory it was given (the device
sanitizer and debuggers are not available to it).

An `Arena` places every operand of a call inside a larger allocation of its
own, with a band of sentinel words in front and behind:

    [ slack | front band | operand (rows x ld, gap columns are band) | back band ]

  * a band is max(4096, 128 * ld) words: one full tile of the largest row tile
    in the library (128 rows) at the operand's leading dimension;
  * with ld > cols the columns [cols, ld) of every row, the last row's
    included, belong to the band ("gap");
  * the operand starts 256-byte aligned, plus `skew_bytes`;
  * float bands hold the NaN 0x7FC0A5A5 (float64: 0x7FF8A5A5A5A5A5A5): not the
    canonical NaN, so a kernel that stores a NaN of its own is still seen;
    integer bands hold a value that is VALID where the kernel would read it
    (`fill=(a, b)`, e.g. (Q - 1, 0) for codes): no band ever holds a word
    that could send a load or a store to a wild address, so a guard test
    cannot fault the device;
  * bands are compared as integers, bit for bit.

`check()` finds WRITES outside an operand.  READS are found by `read_check`:
the entry runs with bands A (NaN for floats that only feed arithmetic), then
with bands B (0.0; the second in-range value for index-like operands), and
every output must have the same bits both times.

KNOWN LIMIT: a read past an operand that changes no result -- a value that is
loaded and then masked out, multiplied by an exact zero row of weights on
both fills, or selected away -- is invisible to this check.  So is a write of
exactly the word the band already holds.

Works on any torch device (tests/test_guard_host.py plants faults on the CPU).
"""
import numpy as np
import torch

NAN32 = 0x7FC0A5A5                       # band pattern, float32
NAN64 = 0x7FF8A5A5A5A5A5A5               # band pattern, float64
BODY32 = 0x7FC0B6B6                      # initial contents of an output
BODY64 = 0x7FF8B6B6B6B6B6B6
ALIGN = 256
MIN_BAND = 4096                          # words
TILE_ROWS = 128                          # the largest row tile in the library

_INT_OF = {torch.float32: torch.int32, torch.int32: torch.int32,
           torch.float64: torch.int64, torch.int64: torch.int64}


def _bits_of(value, dtype):
    """The integer whose bits are `value` in `dtype`."""
    if dtype == torch.float32:
        return int(np.array([value], np.float32).view(np.int32)[0])
    if dtype == torch.float64:
        return int(np.array([value], np.float64).view(np.int64)[0])
    return int(value)


def _signed(pattern, bits):
    return pattern - (1 << bits) if pattern >= 1 << (bits - 1) else pattern


class GuardError(AssertionError):
    """A band was touched (band 'front' / 'back' / 'gap') or an output
    depends on what a band holds (band 'read').  offset, in words of the
    operand's dtype: front: -1 is the word just before the operand; back: +1
    is the first word past its end; gap: (row, column); read: the flat index
    inside the output whose bits changed.  count: words affected."""

    def __init__(self, operand, band, offset, count, detail=''):
        self.operand, self.band = operand, band
        self.offset, self.count = offset, count
        AssertionError.__init__(
            self, 'operand %r: %s band, first changed word at offset %s, '
            '%d word(s) changed%s' % (operand, band, offset, count, detail))


class _Operand(object):
    pass


class Arena(object):
    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        self.ops = {}                    # name -> _Operand, in placing order
        self.variant = 'A'

    # ------------------------------------------------------------- placing
    def place(self, name, data_or_shape, dtype=torch.float32, ld=None,
              role='in', skew_bytes=0, fill=None, tile_ld=None):
        """A tensor of the given shape (or holding `data`) inside a guarded
        allocation.  ld: words between rows of the LAST dimension's rows
        (all leading dimensions are flattened into rows); the returned tensor
        is then the strided [rows, cols] view.  role: 'in' (bands are
        refilled by `refill`), 'out', 'inout'.  fill=(a, b): the band values
        of variants A and B for operands whose values become indices or
        addresses; default (NaN pattern, 0.0) for floats, (0, 0) for ints.
        tile_ld: the row length the bands are sized for where `ld` is not one
        (planes of [rows][32] placed `ld` words apart: tile_ld=32, so that
        every plane has bands of its own in the gap to the next)."""
        assert name not in self.ops, name
        assert role in ('in', 'out', 'inout'), role
        data = None
        if isinstance(data_or_shape, (tuple, list, torch.Size)):
            shape = tuple(int(s) for s in data_or_shape)
        elif isinstance(data_or_shape, int):
            shape = (data_or_shape,)
        else:
            data = torch.as_tensor(np.ascontiguousarray(data_or_shape)
                                   if isinstance(data_or_shape, np.ndarray)
                                   else data_or_shape).to(dtype)
            shape = tuple(data.shape)
        idt = _INT_OF[dtype]
        isz = 4 if idt == torch.int32 else 8
        assert skew_bytes % isz == 0 and 0 <= skew_bytes < ALIGN
        cols = shape[-1] if shape else 1
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        if ld is None:
            ld_ = cols
        else:
            ld_ = int(ld)
            assert ld_ >= cols, (ld_, cols)
        span = rows * ld_ if ld is not None else rows * cols
        band = max(MIN_BAND, TILE_ROWS * (ld_ if tile_ld is None else
                                          int(tile_ld)))
        total = band + span + band
        raw8 = torch.empty(total * isz + 2 * ALIGN, dtype=torch.uint8,
                           device=self.device)
        base = raw8.data_ptr()
        start = (-(base + band * isz)) % ALIGN + skew_bytes
        assert start % isz == 0
        words = raw8[start:start + total * isz].view(idt)
        assert (words.data_ptr() + band * isz) % ALIGN == skew_bytes

        op = _Operand()
        op.name, op.dtype, op.role = name, dtype, role
        op.raw8, op.words = raw8, words
        op.band, op.span, op.rows, op.cols, op.ld = band, span, rows, cols, ld_
        is_f = dtype in (torch.float32, torch.float64)
        if fill is None:
            fill = ((_signed(NAN32, 32) if isz == 4 else _signed(NAN64, 64))
                    if is_f else 0, 0.0 if is_f else 0)
            op.fill_bits = (fill[0], _bits_of(fill[1], dtype) if is_f else 0)
        else:
            op.fill_bits = tuple(_bits_of(v, dtype) for v in fill)
        # band word indices (into `words`), in ascending order
        dev = self.device
        idx = [torch.arange(0, band, device=dev)]
        if ld is not None and ld_ > cols:
            r = torch.arange(rows, device=dev).reshape(-1, 1) * ld_
            c = torch.arange(cols, ld_, device=dev).reshape(1, -1)
            idx.append((band + r + c).reshape(-1))
        idx.append(torch.arange(band + span, total, device=dev))
        op.band_idx = torch.cat(idx)
        op.expect = torch.full((op.band_idx.numel(),), op.fill_bits[0],
                               dtype=idt, device=self.device)
        words[op.band_idx] = op.expect
        body = words[band:band + span].view(dtype)
        if ld is not None:
            t = torch.as_strided(body, (rows, cols), (ld_, 1))
        else:
            t = body.view(shape)
        if data is not None:
            t.copy_(data.reshape(t.shape).to(self.device))
        elif is_f:
            t.view(idt).fill_(_signed(BODY32, 32) if isz == 4
                              else _signed(BODY64, 64))
        else:
            t.fill_(op.fill_bits[0])
        op.tensor = t
        op.initial = t.clone()
        self.ops[name] = op
        return t

    def __getitem__(self, name):
        return self.ops[name].tensor

    def ptr(self, name):
        return None if name is None else self.ops[name].tensor.data_ptr()

    # ------------------------------------------------------------ checking
    def refill(self, variant):
        """Bands of 'in' and 'inout' operands get contents 'A' or 'B'."""
        k = {'A': 0, 'B': 1}[variant]
        self.variant = variant
        for op in self.ops.values():
            if op.role == 'out':
                continue
            op.expect.fill_(op.fill_bits[k])
            op.words[op.band_idx] = op.expect

    def commit(self, name):
        """What operand `name` holds now is what `reset` restores (an input
        that a set-up launch computed)."""
        op = self.ops[name]
        op.initial = op.tensor.clone()

    def reset(self):
        """Every operand back to the contents it was placed with."""
        for op in self.ops.values():
            op.tensor.copy_(op.initial)

    def check(self):
        """Every band of every operand, inputs included, is intact."""
        for op in self.ops.values():
            got = op.words[op.band_idx]
            bad = got != op.expect
            n = int(bad.sum())
            if n == 0:
                continue
            first = int(op.band_idx[bad][0])
            at = first - op.band
            if at < 0:
                band, off = 'front', at
            elif at >= op.span:
                band, off = 'back', at - op.span + 1
            else:
                band, off = 'gap', (at // op.ld, at % op.ld)
            w = int(op.words[first])
            raise GuardError(op.name, band, off, n,
                             ' (bands %s; word now 0x%x)'
                             % (self.variant, w & ((1 << (64 if op.words.
                                                   dtype == torch.int64
                                                   else 32)) - 1)))

    def outputs(self):
        return [op for op in self.ops.values() if op.role != 'in']

    def snapshot(self):
        """The bits of every 'out' / 'inout' operand."""
        return {op.name: op.tensor.clone().view(_INT_OF[op.dtype])
                for op in self.outputs()}

    def untouched(self):
        """Every operand still holds what it was placed with (an entry that
        returned an error before any launch)."""
        for op in self.ops.values():
            idt = _INT_OF[op.dtype]
            bad = op.tensor.view(idt) != op.initial.view(idt)
            n = int(bad.sum())
            if n:
                at = int(torch.nonzero(bad.reshape(-1))[0])
                raise GuardError(op.name, 'body', at, n,
                                 ' (expected untouched)')


def _sync(arena):
    if arena.device.type == 'cuda':
        torch.cuda.synchronize()


def read_check(arena, run):
    """Run `run()` with bands A, then with bands B on restored operands:
    every band intact after each run, every output's bits equal between the
    two.  Returns the outputs' bits of the first run."""
    arena.refill('A')
    arena.reset()
    run()
    _sync(arena)
    arena.check()
    first = arena.snapshot()
    arena.refill('B')
    arena.reset()
    run()
    _sync(arena)
    arena.check()
    second = arena.snapshot()
    for name, a in first.items():
        bad = a != second[name]
        n = int(bad.sum())
        if n:
            at = int(torch.nonzero(bad.reshape(-1))[0])
            raise GuardError(name, 'read', at, n,
                             ': the output differs between band contents A '
                             'and B, so something outside an operand was read')
    arena.refill('A')
    return first
