#!/bin/bash
# Register / spill / scratch / LDS use of every kernel of every unit that the Makefile compiles with HIPFLAGS (its <unit>_f64.o objects:
# npb_kernels.hip, npb_attachments.hip, npb_storage_free.hip; add -DNPB_BUILD_F32 as $1 for the fp32-storage build, the <unit>_f32.o
# objects).  The units come from `make print-objects`.  No GPU needed.
cd "$(dirname "$0")/../nuclear_sim_amd/csrc" || exit 1
suffix=_f64.o
[ "$1" = "-DNPB_BUILD_F32" ] && suffix=_f32.o
for unit in $(make -s print-objects | grep -- "$suffix\$" | sed "s/$suffix\$/.hip/"); do
  echo "== $unit"
  /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -freciprocal-math -fapprox-func \
    -fvisibility=hidden $1 --cuda-device-only -Rpass-analysis=kernel-resource-usage -c -o /dev/null "$unit" 2>&1 |
    awk '/Function Name:/ {name=$0; sub(/.*Function Name: /,"",name); sub(/ \[-Rpass.*/,"",name); gsub(/^_Z[0-9]+/,"",name); sub(/12npb_params_t.*|mPd$|iimPKdPd$|PKdm.*|Pdm.*/,"",name)}
         / VGPRs:/ {v=$(NF-1)} / AGPRs:/ {a=$(NF-1)} /SGPRs Spill/ {ss=$(NF-1)} /VGPRs Spill/ {vs=$(NF-1)} /ScratchSize/ {sc=$(NF-1)}
         /Occupancy/ {oc=$(NF-1)} /LDS Size/ {printf "%-28s VGPR %3s AGPR %3s  SGPR-spill %4s VGPR-spill %3s scratch %5s B/lane  occupancy %s  LDS %s B\n", name, v, a, ss, vs, sc, oc, $(NF-1)}'
done
