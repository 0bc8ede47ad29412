#!/bin/bash
# Build an alternative libc12381_hip.so with extra compile flags into crypto12381_amd/lib/exp/lib<name>.so (A/B runs: C12381_LIB).
# usage: bash tools/build_variant.sh <name> <extra flags...>      e.g.  bash tools/build_variant.sh dflt BASEFLAGS=... (the compile-time A/B knobs of
# rounds 2-4 are gone from the sources with their losing arms: a variant is a working-tree edit built under another name, or other compiler flags)
# (add -DC12381_EXPERIMENTS for a variant that also reads the C12381_* tuning variables; BASEFLAGS="..." in the environment replaces the
# product's base flags for every unit, e.g. to drop the max-ilp scheduling strategy; CSRC=<dir> builds another checkout's csrc/ — the
# parent commit's, for an A/B of a change against what it replaces)
# The translation units and each unit's flags are the product's: crypto12381_amd/build.py (UNITS, unit_cflags).
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=${CSRC:-$ROOT/crypto12381_amd/csrc}
OUT=$ROOT/crypto12381_amd/lib/exp; OBJ=$OUT/obj_$NAME
mkdir -p $OBJ
for f in "$@"; do case "$f" in *amdgpu-use-amdgpu-trackers*) echo "refused: $f (docs/lab_notes.md 5b)"; exit 2;; esac; done
# one line per unit: name, then its flags (build.py is read as a file: importing the package would load the library)
PLAN=$(python3 -c "
import importlib.util, sys
spec = importlib.util.spec_from_file_location('c12381_build', sys.argv[1]); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
for u in b.UNITS: print(u[:-4], *b.unit_cflags(u))" $ROOT/crypto12381_amd/build.py)
pids=""
while read -r u UF; do
  /opt/rocm/bin/hipcc ${BASEFLAGS:-$UF} "$@" -c -o $OBJ/$u.o $CSRC/$u.hip 2> $OBJ/$u.err &
  pids="$pids $!"
done <<< "$PLAN"
for p in $pids; do wait $p || { cat $OBJ/*.err; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/lib$NAME.so $OBJ/*.o
rm -rf $OBJ
ls -la $OUT/lib$NAME.so
