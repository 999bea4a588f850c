"""Fingerprint the gfx950 code of the persistent residual-stack kernels.

Extracts the device code object of csrc/wn_stack.hip from the built object
file, disassembles it with llvm-objdump and prints, per kernel, the number of
instructions and a SHA-256 of the instruction text (addresses and encodings
stripped; branch offsets are relative already).  Two builds whose lines agree
run the same machine code in those kernels.

The local-conditioning launches are separate instantiations of the 32-row
kernels (an extra StackLc argument); the fingerprints of every other kernel
must not change when they do.

    python tools/stack_disasm.py [build/wn_stack.o] [--dump DIR]

--match REGEX fingerprints the kernels whose names match REGEX instead (any
object; --exclude REGEX drops names), e.g. the fast-generation kernels
without their local-conditioning variants (profiles/fastgen_disasm_lc.txt):

    python tools/stack_disasm.py build/wn_fastgen.o --match 'kernel' \
        --exclude '_lc_' --strip-padding

--strip-padding drops the run of s_nop after a kernel's last instruction:
the padding up to the next function in the code object, which depends on
what follows the kernel, not on its code.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OBJ = os.path.join(ROOT, 'tensorflow-wavenet_amd', 'build', 'wn_stack.o')
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def disassemble(obj):
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fatbin')
        co = os.path.join(tmp, 'dev.co')
        subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'),
                               '--dump-section=.hip_fatbin=' + fat, obj])
        subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'),
                               '--unbundle', '--type=o', '--input=' + fat,
                               '--targets=' + TARGET, '--output=' + co])
        return subprocess.check_output(
            [os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn',
             '-C', co], text=True)


def kernels(text, match=None, exclude=None):
    """{name: [normalised instruction lines]} for every stack kernel (or
    every kernel whose name matches `match` and not `exclude`)."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.*)>:$', line)
        if m:
            name = m.group(1)
            cur = None
            if match is None:
                want = 'stack_' in name and '_kernel' in name
            else:
                want = re.search(match, name) is not None
            if exclude is not None and re.search(exclude, name):
                want = False
            if want:
                cur = out.setdefault(name, [])
            continue
        if cur is None:
            continue
        ins = line.split('//')[0].strip()
        if ins:
            cur.append(re.sub(r'\s+', ' ', ins))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('obj', nargs='?', default=DEFAULT_OBJ)
    ap.add_argument('--dump', default=None,
                    help='also write each kernel\'s normalised text here')
    ap.add_argument('--match', default=None,
                    help='regex of the kernel names to fingerprint '
                         '(default: the stack kernels)')
    ap.add_argument('--exclude', default=None,
                    help='regex of kernel names to leave out')
    ap.add_argument('--strip-padding', action='store_true',
                    help='drop the s_nop padding after each kernel')
    args = ap.parse_args(argv)
    ks = kernels(disassemble(args.obj), args.match, args.exclude)
    if args.strip_padding:
        for body in ks.values():
            while body and body[-1] in ('s_nop 0', '...'):
                body.pop()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for name in sorted(ks):
        body = '\n'.join(ks[name]) + '\n'
        print('%s %6d %s' % (hashlib.sha256(body.encode()).hexdigest()[:16],
                             len(ks[name]), name))
        if args.dump:
            fn = re.sub(r'[^A-Za-z0-9_]+', '_', name).strip('_') + '.s'
            with open(os.path.join(args.dump, fn), 'w') as f:
                f.write(body)
    return 0


if __name__ == '__main__':
    sys.exit(main())
