#!/bin/bash
# build two variants of the library for tools/ab_lib.sh:
#   tools/mk_ab.sh [-r REV] <file.hip>...
#     -> build/ab/lib_base.so (the named files as of REV, default HEAD)
#        build/ab/lib_new.so  (the named files of the working tree)
# A file that one side lacks is left out of that side, so a split or a merge
# of sources is compared by naming every file involved:
#   tools/mk_ab.sh -r HEAD~1 wn_misc.hip wn_loss.hip wn_optim.hip wn_lc.hip
# Every other object comes from build/ (run the build first).
set -e
PK=tensorflow-wavenet_amd
REV=HEAD
if [ "$1" = "-r" ]; then REV=$2; shift 2; fi
[ $# -gt 0 ] || set -- wn_stack.hip
S=$(mktemp -d)
trap 'rm -rf $S' EXIT
mkdir -p $PK/build/ab $S/base
rm -f $PK/build/ab/lib_*.so
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC"
# per-source flags, as the build gives them
extra() { [ "$1" = wn_fastgen.hip ] && echo -fno-slp-vectorize || true; }
git show $REV:$PK/csrc/wn_common.h > $S/base/wn_common.h
# (.inc: kernel bodies a source includes, as of REV beside the base sources)
for I in $(git ls-tree --name-only $REV $PK/csrc/ | grep '\.inc$' || true); do
  git show $REV:$I > $S/base/$(basename $I)
done
OTHERS=$(ls $PK/build/*.o)
BASE= NEW=
for F in "$@"; do
  N=${F%.hip}
  OTHERS=$(echo "$OTHERS" | grep -v "/$N.o" || true)
  if git cat-file -e $REV:$PK/csrc/$F 2>/dev/null; then
    git show $REV:$PK/csrc/$F > $S/base/$F
    /opt/rocm/bin/hipcc $FL $(extra $F) -c $S/base/$F -o $S/base_$N.o
    BASE="$BASE $S/base_$N.o"
  fi
  if [ -f $PK/csrc/$F ]; then
    /opt/rocm/bin/hipcc $FL $(extra $F) -c $PK/csrc/$F -o $S/new_$N.o
    NEW="$NEW $S/new_$N.o"
  fi
done
/opt/rocm/bin/hipcc $FL -shared -o $PK/build/ab/lib_base.so $BASE $OTHERS
/opt/rocm/bin/hipcc $FL -shared -o $PK/build/ab/lib_new.so $NEW $OTHERS
ls -la $PK/build/ab/
