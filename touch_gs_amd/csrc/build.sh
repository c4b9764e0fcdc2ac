#!/bin/bash
# Builds libtgs_hip.so for gfx950 in-tree (touch_gs_amd/lib/).  hipcc cross-compiles without a GPU.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wall -Wno-unused-function $TGS_EXTRA_FLAGS"
SRCS="api project binning raster optim imgloss depthcorr depthnormal exposure gpis tsdf peer mcmc knn bilagrid"
# raster.hip: the SLP vectoriser pairs the per-pixel FMAs into v_pk_fma_f32, which on gfx950 costs
# 1.84x a plain v_fma_f32 and needs register-pair shuffles (v_mov) around it: K7 127 -> 100 VGPRs and
# -7 % time, K6 -3 % without it (measured, same box)
# imgloss.hip: the same for the SSIM filters (k_ssim_fwd 2105 static VALU with 341 v_pk_* and 326 v_mov at 110
# VGPRs -> 2232 VALU, 143 v_mov, 92 VGPRs: 58.4 -> 51.8 us at 1080p, k_ssim_bwd unchanged; same box, same checksum).
# The other translation units hold HBM-bound kernels: no difference either way (1.0129 / 1.0122 ms per step).
# project.hip: -ffp-contract=on (fusion per source expression, decided by the front end) instead of =fast (decided by
# the backend after inlining): geom_eval / project_fwd_core are inlined into the stand-alone K1 AND into the fused
# optimizer kernel (front prefetch), and the two must produce the same bits.
# depthnormal.hip: -ffp-contract=on for the same reason: dnorm_centre is inlined into the forward and the gradient kernel,
# which must form the same normals and decide |m| > 0 alike.
# exposure.hip: -ffp-contract=on for the same reason: expo_apply is inlined into the forward and into the backward, which
# recomputes the compensated image instead of reading it and must form the bits SSIM saw, so that sign() decides alike.
# tsdf.hip: -ffp-contract=off: every product and sum rounds on its own, as the fp32 NumPy emulation of tests/tsdf_ref.py
# evaluates them (the emulation's measured error is then the kernel's); the kernels are HBM-bound.
# mcmc.hip: -ffp-contract=off for the same reason (tests/mcmc_ref.py emulates the noise term); the Adam update inside it is
# adam1's explicit fmaf chain whatever the flag, which keeps it bit-identical to K9.
# knn.hip: -ffp-contract=off for the same reason (tests/knn_ref.py forms d2 in fp32 NumPy and the GPU test asks for equal bits).
# bilagrid.hip: -ffp-contract=off for the same reason (tests/bilagrid_ref.py forms the cell coordinates in fp32 NumPy), and
# because bg_axis / bg_guide / bg_slice are inlined into the forward and into the backward, which recomputes the cell and the
# corrected image and must form the forward's bits, so that a pixel lands in the same cell and sign() decides alike.
declare -A EXTRA=([raster]="-fno-slp-vectorize" [imgloss]="-fno-slp-vectorize" [project]="-ffp-contract=on"
                  [depthnormal]="-ffp-contract=on" [exposure]="-ffp-contract=on" [tsdf]="-ffp-contract=off" [mcmc]="-ffp-contract=off" [knn]="-ffp-contract=off" [bilagrid]="-ffp-contract=off")
pids=()
for s in $SRCS; do
  [ -f "$HERE/$s.hip" ] || continue
  stale=0
  [ -f "$OUT/$s.o" ] || stale=1
  for dep in "$HERE/$s.hip" "$HERE"/*.h "$HERE/../../include/tgs.h" "$0"; do
    [ "$dep" -nt "$OUT/$s.o" ] && stale=1
  done
  if [ $stale = 1 ]; then
    $HIPCC $FLAGS ${EXTRA[$s]} -c "$HERE/$s.hip" -o "$OUT/$s.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
OBJS=""
for s in $SRCS; do [ -f "$OUT/$s.o" ] && OBJS="$OBJS $OUT/$s.o"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT/libtgs_hip.so"
echo "built $OUT/libtgs_hip.so"
