#!/bin/bash
# tools/isa_exec_spills.py over every instantiation of the current build (CPU only: hipcc -S per object, 8 at a time).
# usage: tools/lint_all.sh out.txt
out=${1:-/tmp/lint_all.txt}
cd "$(dirname "$0")/.."
tmp=$(mktemp -d)
list=""
for s in $(seq 2 32); do for h in 1 2 4; do for e in 0 1; do list="$list $s,$h,$e"; done; done; done
for s in $(seq 2 16); do for e in 0 1; do list="$list $s,8,$e"; done; done
for s in $(seq 2 16); do list="$list $s,0,0"; done  # (H = 0: the screened variant without window history)
one() { IFS=, read s h e <<< "$1"; extra=""; 
  if [ $e = 1 ] && { [ $h = 8 ] || { [ $s -ge 17 ] && [ $h -ge 2 ]; } || { [ $s -ge 11 ] && [ $h = 4 ]; }; }; then extra="-mllvm -amdgpu-spill-sgpr-to-vgpr=0"; fi
  tools/isa_dump.sh $s $h $e $2/k_${s}_${h}_${e}.s $extra > /dev/null 2>&1
  python3 tools/isa_exec_spills.py $2/k_${s}_${h}_${e}.s --sites 0 | sed "s/^k_/S,H,E = /"
  python3 tools/isa_lane_loss.py $2/k_${s}_${h}_${e}.s --sites 3 | sed "s/^k_/LANES S,H,E = /" >> $2/lanes.txt; rm -f $2/k_${s}_${h}_${e}.s; }
export -f one
echo $list | tr ' ' '\n' | grep . | xargs -P 8 -I{} bash -c "one {} $tmp" > $out.unsorted
sort -t_ -k2,2n -k3,3n -k4,4n $out.unsorted > $out; rm -f $out.unsorted; cp $tmp/lanes.txt $out.lanes; rm -f $tmp/lanes.txt
# the other translation units: the time-tiled kernels and the parallel fit (psk_tile.hip), the reference-order kernel (psk_kernels.hip),
# the instantiated front stages (psk_tile_inst.hip, samplesPerBaud 2 ... 16)
FL="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wno-unused-function -Iinclude -Ipsk_soft_amd/csrc --cuda-device-only -S"
others() { f=$1; shift; /opt/rocm/bin/hipcc $FL "$@" -o $tmp/$f.s psk_soft_amd/csrc/${f%%@*}.hip 2>/dev/null
  python3 tools/isa_exec_spills.py $tmp/$f.s --sites 0 >> $out; python3 tools/isa_lane_loss.py $tmp/$f.s --sites 3 >> $out.lanes; rm -f $tmp/$f.s; }
others psk_tile; others psk_kernels
for s in $(seq 2 16); do others psk_tile_inst@S$s -DPSK_INST_S=$s -DPSK_INST_H=1; done
# the builds that read a packet format in place (PSK_INST_PKT=cs16 | cs8 | cf16): the wave-scan kernel for numAvg <= 128, samplesPerBaud
# 2 ... 16, both tiers; the reference-order kernel; and the conversion pre-passes of the three (psk_pkt.hip)
for f in cs16 cs8 cf16; do
  for s in $(seq 2 16); do for e in 0 1; do others psk_fast_inst@${f}_S${s}_H1_E$e -DPSK_INST_PKT=$f -DPSK_INST_S=$s -DPSK_INST_H=1 -DPSK_INST_E=$e; done; done
  others psk_kernels@$f -DPSK_INST_PKT=$f
done
others psk_pkt
# wide symbols (samplesPerBaud > 1024): the chunk and pick kernels (psk_wide.hip), the reference-order kernel's PSK_SEQ_WIDE build
others psk_wide; others psk_kernels@wide -DPSK_SEQ_WIDE=1
# the reduction pass of PSK_SOFT_OPT_QUALITY (psk_quality.hip): fold and join
others psk_quality
# the gather pre-pass of psk_soft_process_device_strided (psk_gather.hip): the tile kernel and the plain strided gather, three sample sizes each
others psk_gather
# the tune pre-pass of psk_soft_process_device_tuned (psk_tune.hip): one kernel, the four formats behind a switch
others psk_tune
# the resample pre-pass of psk_soft_process_device_resampled (psk_resample.hip): one kernel, the four formats behind a switch
others psk_resample
# the filter pre-pass of psk_soft_process_device_filtered (psk_fir.hip): one kernel, the four formats and three blockings behind switches
others psk_fir
# the far fit (PSK_SOFT_OPT_FAR_FIT, psk_farfit.hip): the fit stage and the quiet call with the fit window in device memory
others psk_farfit
# the symbol-rate pass of psk_soft_symrate_device (psk_symrate.hip): fold and join
others psk_symrate
echo "instantiations with D sites / with E sites (tools/isa_lane_loss.py):"; grep -c "no covering save) [1-9]" $out.lanes; grep -c "mask restore) [1-9]" $out.lanes
grep -c . $out; grep -v "C (lane carrier moved under a partial mask) 0" $out | wc -l
rmdir $tmp
