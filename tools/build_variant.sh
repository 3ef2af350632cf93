#!/bin/bash
# tools/build_variant.sh NAME "-DFLAG=.. -DFLAG2=.." : an A/B build of the library with extra macros, by csrc/Makefile
# with its flags, into pfb_clean_amd/libpfb_hip_NAME.so (use with PFB_HIP_LIB=... / tools/ab_conv.py).  Prints the
# register / scratch use of the kernels matching $3 (a regex on the demangled name).
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2; PAT=${3:-NONE}
T=/tmp/pfb_variant_$NAME; rm -rf $T; mkdir -p $T
make -s -C pfb_clean_amd/csrc -j"${MAX_JOBS:-8}" -Otarget OBJDIR=$T EXTRA="$FLAGS -Rpass-analysis=kernel-resource-usage" \
    OUT=../libpfb_hip_$NAME.so 2> $T/kres.log
python3 tools/kres.py $T/kres.log "$PAT"
