#!/bin/bash
# CPU-only: psk_soft_symrate_host and psk_soft_symrate_derive (psk_capi.cpp, psk_symrate.h) under AddressSanitizer +
# UndefinedBehaviorSanitizer, called by a stand-alone program with its own main (tools/micro/symrate_host_check.cpp): the host
# side of psk_capi.cpp rebuilt with the sanitizers (device code untouched, -fno-gpu-sanitize), linked with the other objects of
# the current build into an executable in a temporary directory.  The library in the tree is not touched.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap "rm -rf $T" EXIT
cd $R/psk_soft_amd/csrc
make -j8 > /dev/null
SAN="-fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include -I. $SAN -x hip -c psk_capi.cpp -o $T/psk_capi.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include $SAN -x c++ -c $R/tools/micro/symrate_host_check.cpp -o $T/check.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 $SAN -o $T/symrate_host_check $T/check.o $T/psk_capi.o $(ls obj/*.o | grep -v -e psk_capi.o -e dev_prims.o -e prepass_probe.o)
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $T/symrate_host_check | tail -3
