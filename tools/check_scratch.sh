#!/bin/bash
# Register / scratch use of the kernels the BASELINE configs launch (hipcc -Rpass-analysis=kernel-resource-usage on the two
# of fftconv_pow2.hip's three objects that hold them -- the power-of-two rows and columns -- and on cgvec.hip / wavelet.hip,
# built by csrc/Makefile with its flags) and of every instantiation of the mask pass that comps.hip and spi.hip share
# (pixmask.hpp); exits non-zero if one of them uses scratch.
#   tools/check_scratch.sh [output.md]
set -e
cd "$(dirname "$0")/.."
T=/tmp/pfb_kres; rm -rf $T; mkdir -p $T
make -s -C pfb_clean_amd/csrc -j4 -Otarget OBJDIR=$T EXTRA=-Rpass-analysis=kernel-resource-usage \
    $T/fftconv_pow2.o $T/fftconv_pow2_col.o $T/cgvec.o $T/wavelet.o $T/comps.o $T/spi.o 2> $T/kres.log
PAT='k_row_fwd_pow2q<float, 2048, false>|k_col_pow2p<float, 4096, 8, true, true>|k_row_inv_pow2p<float, 2048, 8, 2, false>|k_pcg_update_dir<(float|double), ., 2, true, true>|k_row_fwd_pow2<float, (512|1024), (8|16)>|k_col_pow2<float, 1024, 4>|k_row_inv_pow2<float, 512, 8>|k_col_pow2p<float, 2048, 8, false, (true|false)>|k_row_inv_pow2p<float, 1024, 8, 0, false>|k_row_fwd_pow2<double, 4096, 8>|k_col_pow2x<double, 8192, 8, true>|k_row_inv_pow2p<double, 4096, 16, 2, false>|k_col_pow2x<float, 8192, 8, true>|k_row_fwd_pow2q<float, 4096, false>|k_row_inv_pow2p<float, 4096, 16, 2, false>|k_dual_update_vec<float, 4, true>|k_dwt_l1_fused<float|k_idwt_finest_fused2<float|k_pd_primal_vec<float, 4>|k_dwt_batched<float|k_idwt_batched2<float|k_pixmask<|k_count_scan<'
{
  echo "# kernel resources of the BASELINE configs' kernels (\`tools/check_scratch.sh\`: hipcc -Rpass-analysis=kernel-resource-usage)"
  echo; echo '```'
  python3 tools/kres.py $T/kres.log "$PAT"
  echo '```'
} > ${1:-/dev/stdout}
bad=$(python3 tools/kres.py $T/kres.log "$PAT" | awk '{ if ($(NF-2) != 0) print }')
if [ -n "$bad" ]; then echo "kernels with scratch:"; echo "$bad"; exit 1; fi
echo "no scratch in the listed kernels"
