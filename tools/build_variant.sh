#!/bin/bash
# usage: tools/build_variant.sh [--unit UNIT | --gemm] <name> [-DFOO=1 ...]   -> tools/ab/lib<name>.so
#   UNIT, a translation unit of fpqvar_amd/csrc (default fpq_kernels; --gemm = --unit fpq_gemm), rebuilt with the defines and the
#   regular flags of __graft_entry__.py; fpq_build_tag.hip rebuilt with the tag <name>; every other unit's object reused from the
#   last regular build.  Where the switches act: -DFPQ_FAST16_U / -DFPQ_FAST16_HW4_U: fpq_kernels; -DFPQ_ADALN_STAMPS /
#   -DFPQ_ADALN_TIGHT: fpq_adaln; -DFPQ_ISA_CENSUS: fpq_rotate and fpq_adaln (fpq_rotate_mfma.h); -DFPQ_GEMM6_STAMPS: fpq_gemm.
set -e
tu=fpq_kernels
if [ "$1" = --gemm ]; then tu=fpq_gemm; shift; elif [ "$1" = --unit ]; then tu=${2%.hip}; shift 2; fi
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/fpqvar_amd/csrc
[ -f $csrc/$tu.hip ] || { echo "no translation unit $csrc/$tu.hip" >&2; exit 1; }
# the regular build's flags, this unit's own ones and every unit in link order (__graft_entry__.py)
g() { (cd $root && python -c "import __graft_entry__ as g, os; print($1)"); }
base=$(g "' '.join(g.HIP_FLAGS)")
extra=$(g "' '.join(g.EXTRA_FLAGS.get('$tu.hip', []))")
units=$(g "' '.join(os.path.basename(s)[:-4] for s in g.HIP_SRCS)")
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT
/opt/rocm/bin/hipcc $base $extra "$@" -c -o $tmp/$tu.o $csrc/$tu.hip 2>/dev/null
/opt/rocm/bin/hipcc $base -DFPQ_BUILD_TAG="\"$name\"" -c -o $tmp/fpq_build_tag.o $csrc/fpq_build_tag.hip
objs=
for u in $units; do
  if [ -f $tmp/$u.o ]; then objs="$objs $tmp/$u.o"; else objs="$objs $csrc/$u.o"; fi
done
mkdir -p $root/tools/ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/tools/ab/lib$name.so $objs
echo built tools/ab/lib$name.so
