# The device BVH build's compile-time constants (bvh_device.h: NB_CHAIN_START, NB_RUN_LEN, NB_KSUB) swept on the bench's
# reference-scene leg: the laboratory library rebuilt with each set of -D flags.   bash tools/bvh_build_sweep.sh ["-DNB_KSUB=1024" ...]
# Without arguments: the nine configurations of profiles/r04_bvh_build_constants.txt.  On the way out, however it ends, the
# laboratory library is rebuilt with the default constants.
set -o pipefail
cd nbody-simulation_amd/csrc || exit 1
export NBODY_HIP_LIBRARY=lab
UNITS="bvh_build bvh_fold bvh_partition bvh_subtrees bvh_finish"  # every unit that includes bvh_device.h
drop_objects() { for u in $UNITS; do rm -f "$u.lab.o"; done; }
trap 'drop_objects; make lab > /dev/null' EXIT
if [ $# -eq 0 ]; then
  set -- "" "-DNB_CHAIN_START=256" "-DNB_CHAIN_START=1024" "-DNB_CHAIN_START=2048" "-DNB_RUN_LEN=8192" "-DNB_RUN_LEN=32768" "-DNB_RUN_LEN=1000000" "-DNB_KSUB=1024" "-DNB_KSUB=4096"
fi
for cfg in "$@"; do
  drop_objects
  make lab DEFS="$cfg" > /dev/null 2>&1 || { echo "build failed: $cfg"; continue; }
  (cd ../.. && timeout -k 10 120 python bench.py --leg reference_scene_bvh --no-cpu-baseline > gpurun_out/r04_bs.json 2> gpurun_out/r04_bs.err && python -c "
import json,sys; d=json.load(open('gpurun_out/r04_bs.json'))
print(repr(sys.argv[1]), 'build_ms', round(d['exact']['build_ms'],4), 'step', round(d['exact']['ms_per_step'],4), 'fast step', round(d['fast']['ms_per_step'],4))
" "$cfg") || echo "run failed: $cfg"
done
