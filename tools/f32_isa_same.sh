#!/bin/bash
# Is the float path's machine code unchanged?  Compiles every wave-scan instantiation of tools/lint_all.sh's list and the
# other translation units (psk_tile.hip, psk_kernels.hip, psk_tile_inst.hip S 2 .. 16) to gfx950 assembly twice -- from the
# working tree and from git ref REF -- and compares the instruction streams with comments, directives, metadata and labels
# stripped.  The complex int16 units are compared too (PSK_INST_CS16=1: the wave-scan kernel for samplesPerBaud 2 .. 16, both
# tiers, the reference-order kernel, the conversion pre-pass psk_cs16.hip): 32 more; the complex int8 units (PSK_INST_CS8=1,
# psk_cs8.hip) and the complex binary16 units (PSK_INST_CF16=1, psk_cf16.hip) the same way.  A unit REF does not have yet (its
# source file or its PSK_INST_* build is missing there) is reported as "new", not compared.  CPU only (hipcc -S), 8 compiles at
# a time.
# usage: tools/f32_isa_same.sh [REF] [out.txt]     (REF defaults to main)
ref=${1:-main}
out=${2:-/tmp/f32_isa_same.txt}
cd "$(dirname "$0")/.."
tmp=$(mktemp -d)
mkdir -p $tmp/old $tmp/new $tmp/s
git archive "$ref" include psk_soft_amd/csrc | tar -x -C $tmp/old
cp -r include psk_soft_amd $tmp/new/ 2>/dev/null
FL="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wno-unused-function --cuda-device-only -S"
# instruction lines only: no comments, directives (.xxx), labels (xxx:), blank lines; symbol names masked
strip() { sed -e 's/;.*$//' -e 's/\/\/.*$//' "$1" | grep -vE '^\s*($|\.|[A-Za-z0-9_.$]+:)' | sed -E 's/_Z[A-Za-z0-9_]+/SYM/g; s/\.L[A-Za-z0-9_]+/LBL/g'; }
export -f strip
one() {  # one TAG FILE [defines...]
    tag=$1; f=$2; shift 2
    def=$(printf '%s\n' "$@" | sed -n 's/^-D\(PSK_INST_C[SF][0-9]*\)=1$/\1/p')
    if [ ! -f $tmp/old/psk_soft_amd/csrc/$f ] || { [ -n "$def" ] && ! grep -q "$def" $tmp/old/psk_soft_amd/csrc/psk_wave.h; }; then
        /opt/rocm/bin/hipcc $FL -I$tmp/new/include -I$tmp/new/psk_soft_amd/csrc "$@" -o $tmp/s/$tag.new.s $tmp/new/psk_soft_amd/csrc/$f 2>$tmp/s/$tag.new.err ||
            { echo "$tag: compile failed (new): $(grep -m1 error $tmp/s/$tag.new.err)"; return 0; }
        echo "$tag: new ($(strip $tmp/s/$tag.new.s | wc -l) instructions)"
        rm -f $tmp/s/$tag.new.s
        return 0
    fi
    for t in old new; do
        /opt/rocm/bin/hipcc $FL -I$tmp/$t/include -I$tmp/$t/psk_soft_amd/csrc "$@" -o $tmp/s/$tag.$t.s $tmp/$t/psk_soft_amd/csrc/$f 2>$tmp/s/$tag.$t.err ||
            { echo "$tag: compile failed ($t): $(grep -m1 error $tmp/s/$tag.$t.err)"; return 0; }
    done
    if cmp -s <(strip $tmp/s/$tag.old.s) <(strip $tmp/s/$tag.new.s); then
        echo "$tag: same ($(strip $tmp/s/$tag.new.s | wc -l) instructions)"
    else
        echo "$tag: DIFFERENT"
    fi
    rm -f $tmp/s/$tag.old.s $tmp/s/$tag.new.s
}
export -f one
export tmp FL
list=""
for s in $(seq 2 32); do for h in 1 2 4; do for e in 0 1; do list="$list $s,$h,$e"; done; done; done
for s in $(seq 2 16); do for e in 0 1; do list="$list $s,8,$e"; done; done
for s in $(seq 2 16); do list="$list $s,0,0"; done
{
    for x in $list; do
        IFS=, read s h e <<< "$x"
        extra=""
        if [ $e = 1 ] && { [ $h = 8 ] || { [ $s -ge 17 ] && [ $h -ge 2 ]; } || { [ $s -ge 11 ] && [ $h = 4 ]; }; }; then
            extra="-mllvm -amdgpu-spill-sgpr-to-vgpr=0"
        fi
        echo "fast_S${s}_H${h}_E${e} psk_fast_inst.hip -DPSK_INST_S=$s -DPSK_INST_H=$h -DPSK_INST_E=$e $extra"
    done
    echo "tile psk_tile.hip"
    echo "kernels psk_kernels.hip"
    for s in $(seq 2 16); do echo "tile_inst_S$s psk_tile_inst.hip -DPSK_INST_S=$s -DPSK_INST_H=1"; done
    for s in $(seq 2 16); do for e in 0 1; do echo "cs16_fast_S${s}_H1_E$e psk_fast_inst.hip -DPSK_INST_CS16=1 -DPSK_INST_S=$s -DPSK_INST_H=1 -DPSK_INST_E=$e"; done; done
    echo "cs16_kernels psk_kernels.hip -DPSK_INST_CS16=1"
    echo "cs16_convert psk_cs16.hip"
    for s in $(seq 2 16); do for e in 0 1; do echo "cs8_fast_S${s}_H1_E$e psk_fast_inst.hip -DPSK_INST_CS8=1 -DPSK_INST_S=$s -DPSK_INST_H=1 -DPSK_INST_E=$e"; done; done
    echo "cs8_kernels psk_kernels.hip -DPSK_INST_CS8=1"
    echo "cs8_convert psk_cs8.hip"
    for s in $(seq 2 16); do for e in 0 1; do echo "cf16_fast_S${s}_H1_E$e psk_fast_inst.hip -DPSK_INST_CF16=1 -DPSK_INST_S=$s -DPSK_INST_H=1 -DPSK_INST_E=$e"; done; done
    echo "cf16_kernels psk_kernels.hip -DPSK_INST_CF16=1"
    echo "cf16_convert psk_cf16.hip"
} | sed "s/ *$//" | xargs -P 8 -L 1 bash -c 'one "$@"' _ | sort > $out
echo "$(grep -c ': same' $out) same, $(grep -c ': new' $out) new, $(grep -c 'DIFFERENT' $out) different, $(grep -c 'failed' $out) failed of $(grep -c . $out)"
[ -n "${KEEP:-}" ] || rm -rf $tmp
