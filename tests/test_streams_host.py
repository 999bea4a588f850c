"""The coverage rule of the stream tests, without a GPU: every wn_* entry of
include/wavenet_hip.h that takes `void* stream` is a row of
tests/test_gpu_guard_entries.py -- tests/test_gpu_streams_abi.py runs every
row on a stalled stream that is not the default stream -- or is named in a
THROUGH_HOST table of the stream modules with the test that runs it through
the host.  A new entry cannot arrive without a stream test.  And
tests/stall.py's bounds."""
import ast
import os
import re

import stall

HERE = os.path.dirname(os.path.abspath(__file__))
MODULES = ('test_gpu_streams_abi', 'test_gpu_streams_training',
           'test_gpu_streams_generation')


def _tables():
    out = {}
    for name in MODULES:
        table = __import__(name).THROUGH_HOST
        assert table, name
        for entry, where in table.items():
            assert entry not in out, entry
            out[entry] = (name, where)
    return out


def test_header_parse_sees_the_stream_argument():
    names = stall.stream_entries()
    assert len(names) >= 100 and len(set(names)) == len(names)
    assert 'wn_fill' in names and 'wn_stack_bwd_lc' in names and \
        'wn_fastgen_batch_step_lc_q' in names
    # queries and host-table builders take no stream
    for n in ('wn_version', 'wn_xent_partials', 'wn_mu_law_thresholds_host',
              'wn_stack_bwd_waves', 'wn_gemm_tn_splits'):
        assert n not in names
    # the handle is always the last argument (stall.spy reads it there)
    src = open(os.path.join(stall.ROOT, 'include', 'wavenet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    for m in re.finditer(r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src):
        if m.group(1) in names:
            last = ' '.join(m.group(2).split(',')[-1].split())
            assert re.match(r'void\s*\*\s*stream$', last), m.group(1)


def test_every_stream_entry_has_a_stream_test():
    import test_gpu_guard_entries as tge
    import test_gpu_streams_abi as abi
    names = set(stall.stream_entries())
    rows = set(r.entry for r in tge.ROWS)
    assert set(p.values[0].entry for p in abi.CASES) == rows
    through = _tables()
    assert not rows & set(through), sorted(rows & set(through))
    unknown = (rows | set(through)) - names
    assert not unknown, 'not entries that take a stream: %s' % sorted(unknown)
    missing = sorted(names - rows - set(through))
    assert not missing, 'entries without a stream test: %s' % missing


def test_the_tables_name_tests_that_exist():
    """'<test function>[<case id>]' (or the wrapper itself in the ABI
    module): the function is defined in the module and the case is one of
    its ids, read from the source."""
    for entry, (module, where) in sorted(_tables().items()):
        src = open(os.path.join(HERE, module + '.py')).read()
        defined = set(n.name for n in ast.walk(ast.parse(src))
                      if isinstance(n, ast.FunctionDef))
        if not isinstance(where, str):           # (wrapper, out=) of the ABI
            assert where[0].__name__ in defined, entry
            assert 'test_wrapped_entry_on_a_stalled_stream' in defined
            continue
        m = re.match(r'(test_\w+)\[(\w+)\]$', where)
        assert m, (entry, where)
        assert m.group(1) in defined, (entry, where)
        assert re.search(r"'%s'" % m.group(2), src), (entry, where)


def test_stall_bounds():
    """No stall is longer than a quarter of the 2 s bounded flag waits of
    the persistent launches, and the rungs end there."""
    assert stall.MAX_MS == 500 and stall.MAX_MS * 4 <= 2000
    assert stall.RUNGS == (10, 40, 160, 500) and max(stall.RUNGS) <= stall.MAX_MS
    assert stall.POOL == 32
    for name in ('wn_stack.hip', 'wn_fastgen.hip'):
        src = open(os.path.join(stall.ROOT, 'tensorflow-wavenet_amd', 'csrc',
                                name)).read()
        assert re.search(r'2 s\b', src), name
