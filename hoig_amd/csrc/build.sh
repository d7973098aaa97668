#!/bin/bash
# Builds libhoig_hip.so (gfx950 code objects) in-tree: hoig_amd/csrc/_build/libhoig_hip.so
set -e
cd "$(dirname "$0")"
mkdir -p _build
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -I../../include -I. -Wno-unused-result -Wno-c++20-designator"
pids=()
for f in conv_igemm conv_igemm_bf16 wgrad_igemm_bf16 dgrad_k128 conv_halo16 conv_wino conv_s2_16 wgrad_dma conv_igemm16 conv_flat16 conv_halo5 wgrad_flat conv_head16 conv_f6 conv_small conv_thin norm attn sample pointwise input_prep raster mano data_prep tuning metrics jpeg pil_resize png png_decode fid_stats grad_guard ema d_augment feature_metrics swd region_metrics; do
  if [ ! -f _build/$f.o ] || [ $f.hip -nt _build/$f.o ] || [ common.h -nt _build/$f.o ] || [ conv_bf16_common.h -nt _build/$f.o ] || [ conv_m16_common.h -nt _build/$f.o ] || [ tuning.h -nt _build/$f.o ] || [ conv_route.h -nt _build/$f.o ] || [ jpeg_entropy.h -nt _build/$f.o ] || [ jpeg_parallel.h -nt _build/$f.o ] || [ pil_resize.h -nt _build/$f.o ] || [ png_deflate.h -nt _build/$f.o ] || [ png_inflate.h -nt _build/$f.o ] || [ fid_stats.h -nt _build/$f.o ] || [ grad_guard.h -nt _build/$f.o ] || [ ema.h -nt _build/$f.o ] || [ d_augment.h -nt _build/$f.o ] || [ feature_metrics.h -nt _build/$f.o ] || [ swd.h -nt _build/$f.o ] || [ region_metrics.h -nt _build/$f.o ] || [ philox.h -nt _build/$f.o ] || [ ../../include/hoig_kernels.h -nt _build/$f.o ]; then
    # input_prep.hip reproduces float->int truncations of the reference: no FMA contraction there (see its header)
    EXTRA=""; { [ $f = input_prep ] || [ $f = raster ] || [ $f = data_prep ] || [ $f = pil_resize ] || [ $f = fid_stats ] || [ $f = grad_guard ] || [ $f = ema ] || [ $f = d_augment ] || [ $f = feature_metrics ] || [ $f = swd ] || [ $f = region_metrics ]; } && EXTRA="-ffp-contract=off"
    $HIPCC $FLAGS $EXTRA -c $f.hip -o _build/$f.o &
    pids+=($!)
  fi
done
# the host half of the JPEG decoder (no HIP call): plain C++ through the same compiler driver, so that it also builds on its own under a
# host sanitizer
if [ ! -f _build/jpeg_host.o ] || [ jpeg_host.cpp -nt _build/jpeg_host.o ] || [ jpeg_entropy.h -nt _build/jpeg_host.o ] || [ jpeg_parallel.h -nt _build/jpeg_host.o ] || [ ../../include/hoig_kernels.h -nt _build/jpeg_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -I../../include -I. -c jpeg_host.cpp -o _build/jpeg_host.o &
  pids+=($!)
fi
# the host half of the Pillow-exact resize (tables and CPU twin, no HIP call); its doubles round step by step
if [ ! -f _build/pil_resize_host.o ] || [ pil_resize_host.cpp -nt _build/pil_resize_host.o ] || [ pil_resize.h -nt _build/pil_resize_host.o ] || [ ../../include/hoig_kernels.h -nt _build/pil_resize_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c pil_resize_host.cpp -o _build/pil_resize_host.o &
  pids+=($!)
fi
# the host half of the PNG encoder (sizes and CPU twins, no HIP call)
if [ ! -f _build/png_host.o ] || [ png_host.cpp -nt _build/png_host.o ] || [ png_deflate.h -nt _build/png_host.o ] || [ ../../include/hoig_kernels.h -nt _build/png_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -I../../include -I. -c png_host.cpp -o _build/png_host.o &
  pids+=($!)
fi
# the host half of the PNG decoder (plan checks, workspace layout and CPU twins, no HIP call)
if [ ! -f _build/png_decode_host.o ] || [ png_decode_host.cpp -nt _build/png_decode_host.o ] || [ png_inflate.h -nt _build/png_decode_host.o ] || [ ../../include/hoig_kernels.h -nt _build/png_decode_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -I../../include -I. -c png_decode_host.cpp -o _build/png_decode_host.o &
  pids+=($!)
fi
# the host half of the fp64 FID statistics (workspace sizes and CPU twins, no HIP call); sums round step by step as on the device
if [ ! -f _build/fid_stats_host.o ] || [ fid_stats_host.cpp -nt _build/fid_stats_host.o ] || [ fid_stats.h -nt _build/fid_stats_host.o ] || [ ../../include/hoig_kernels.h -nt _build/fid_stats_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c fid_stats_host.cpp -o _build/fid_stats_host.o &
  pids+=($!)
fi
# the host half of the gradient guard (workspace size and CPU twins, no HIP call); sums round step by step as on the device
if [ ! -f _build/grad_guard_host.o ] || [ grad_guard_host.cpp -nt _build/grad_guard_host.o ] || [ grad_guard.h -nt _build/grad_guard_host.o ] || [ ../../include/hoig_kernels.h -nt _build/grad_guard_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c grad_guard_host.cpp -o _build/grad_guard_host.o &
  pids+=($!)
fi
# the host half of the weight EMA (CPU twins, no HIP call); every element rounds step by step as on the device
if [ ! -f _build/ema_host.o ] || [ ema_host.cpp -nt _build/ema_host.o ] || [ ema.h -nt _build/ema_host.o ] || [ ../../include/hoig_kernels.h -nt _build/ema_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c ema_host.cpp -o _build/ema_host.o &
  pids+=($!)
fi
# the host half of the discriminator augmentation (CPU twins, no HIP call); every element rounds step by step as on the device
if [ ! -f _build/d_augment_host.o ] || [ d_augment_host.cpp -nt _build/d_augment_host.o ] || [ d_augment.h -nt _build/d_augment_host.o ] || [ philox.h -nt _build/d_augment_host.o ] || [ ../../include/hoig_kernels.h -nt _build/d_augment_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c d_augment_host.cpp -o _build/d_augment_host.o &
  pids+=($!)
fi
# the host half of the feature-space metrics (workspace sizes and CPU twins, no HIP call); sums round step by step as on the device
if [ ! -f _build/feature_metrics_host.o ] || [ feature_metrics_host.cpp -nt _build/feature_metrics_host.o ] || [ feature_metrics.h -nt _build/feature_metrics_host.o ] || [ fid_stats.h -nt _build/feature_metrics_host.o ] || [ ../../include/hoig_kernels.h -nt _build/feature_metrics_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c feature_metrics_host.cpp -o _build/feature_metrics_host.o &
  pids+=($!)
fi
# the host half of the sliced Wasserstein distance (workspace sizes and CPU twins, no HIP call); every value rounds step by step as on
# the device
if [ ! -f _build/swd_host.o ] || [ swd_host.cpp -nt _build/swd_host.o ] || [ swd.h -nt _build/swd_host.o ] || [ philox.h -nt _build/swd_host.o ] || [ ../../include/hoig_kernels.h -nt _build/swd_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c swd_host.cpp -o _build/swd_host.o &
  pids+=($!)
fi
# the host half of the region scores (tap tables, workspace size and CPU twins, no HIP call); the tables' doubles round step by step
if [ ! -f _build/region_metrics_host.o ] || [ region_metrics_host.cpp -nt _build/region_metrics_host.o ] || [ region_metrics.h -nt _build/region_metrics_host.o ] || [ pil_resize.h -nt _build/region_metrics_host.o ] || [ ../../include/hoig_kernels.h -nt _build/region_metrics_host.o ]; then
  $HIPCC -x c++ -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -c region_metrics_host.cpp -o _build/region_metrics_host.o &
  pids+=($!)
fi
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o _build/libhoig_hip.so _build/*.o
echo built _build/libhoig_hip.so
