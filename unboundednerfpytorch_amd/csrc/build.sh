#!/bin/bash
# Build libugrid_hip.so for gfx950 (MI355X).  Usage: csrc/build.sh [extra hipcc flags]
#   UG_OUT=path        alternative output (A/B builds); UG_OBJ=dir its object directory; UG_SHADE_FLAGS / UG_MARCH_FLAGS extra -D
set -e
cd "$(dirname "$0")"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include"
O=${UG_OBJ:-../../build/obj}      # UG_OBJ: separate object directory (parallel A/B builds)
mkdir -p $O
# packed fp32 VALU (v_pk_*_f32 from the SLP vectoriser) issues at half rate on gfx950 and needs extra moves to form
# register pairs: the VALU-bound march kernel is 16 % faster without it, the shade kernel 1.3 %; the grid query
# and the sampling march were part of the march unit and keep its flag (their code was built and measured under it)
NOSLP=-fno-slp-vectorize
# the units of the library, one `name:extra flags` each -- the only list: objects, compiles and the link follow from it
# (ugrid_metrics: an fp64 stencil, -ffp-contract=off is part of its arithmetic contract; ugrid_video: the same for its byte values)
UNITS=(
  "ugrid_ops:"
  "ugrid_update:"
  "ugrid_march:$NOSLP ${UG_MARCH_FLAGS}"
  "ugrid_query:$NOSLP"
  "ugrid_sample:$NOSLP"
  "ugrid_shade:$NOSLP ${UG_SHADE_FLAGS}"
  "ugrid_train:"
  "ugrid_train_mlp:"
  "ugrid_step:"
  "ugrid_metrics:"
  "ugrid_tensorf:"
  "ugrid_frame:"
  "ugrid_video:"
)
OBJS=""
pids=()
for u in "${UNITS[@]}"; do
  name=${u%%:*}
  OBJS="$OBJS $O/$name.o"
  rm -f $O/$name.o               # a failed compile must not link a stale object
  hipcc $FLAGS ${u#*:} -c $name.hip -o $O/$name.o "$@" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done   # a bare `wait` returns 0 even when a job failed
hipcc --offload-arch=gfx950 -shared -fPIC -o ${UG_OUT:-../libugrid_hip.so} $OBJS
# the fp64 twins of the drop-in ops: a library of its own (nothing on the rendering / training path loads it)
# (an A/B build -- UG_OUT set -- gets its own f64 output beside it, so that parallel A/B builds never rewrite the shipped library)
F64_OUT=${UG_OUT_F64:-${UG_OUT:+${UG_OUT%.so}_f64.so}}
hipcc $FLAGS -c ugrid_ops_f64.hip -o $O/ugrid_ops_f64.o "$@"
hipcc --offload-arch=gfx950 -shared -fPIC -o ${F64_OUT:-../libugrid_hip_f64.so} $O/ugrid_ops_f64.o
