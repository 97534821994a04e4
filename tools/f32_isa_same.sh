#!/bin/bash
# Is the machine code unchanged?  Compiles every wave-scan instantiation of tools/lint_all.sh's list and the other translation
# units (psk_tile.hip, psk_kernels.hip, psk_farfit.hip, the pre-passes psk_tune.hip, psk_resample.hip, psk_fir.hip, psk_acquire.hip,
# psk_gather.hip and psk_pkt.hip, psk_tile_inst.hip S 2 .. 16) to gfx950 assembly twice -- from the working tree and from
# git ref REF -- and compares the instruction streams with comments, directives, metadata and labels stripped.  The units of the
# packet formats read in place (cs16, cs8, cf16) are compared too: the wave-scan kernel for samplesPerBaud 2 .. 16, both tiers,
# the reference-order kernel and the conversion kernel of psk_pkt.hip, 32 each.  Either tree may still spell them the old way
# (-DPSK_INST_CS16=1 ..., one psk_<format>.hip per conversion kernel): each side is compiled in its own spelling.  A unit REF
# does not have yet (its source file or its build is missing there) is reported as "new", not compared; one the working tree
# lacks as "failed (no such unit in the working tree)".  A conversion kernel is compared from its label to the end of its
# function only, in both trees -- psk_pkt.hip holds three of them --, so its count is lower than that of the old whole-file
# comparison (139 against 159 for cs16): the 20 lines of kernel metadata (the argument layout), which the filter below lets
# through in a whole file, are not compared for these three units.  CPU only (hipcc -S), 8 compiles at a time.
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
# unit TREE FILE [defines...] -> "FILE defines... [@kernel-regex]" in TREE's spelling, nothing if TREE has no such unit.  A define
# PKT=<format> stands for the format's build of FILE; FILE convert@<format> is the format's conversion kernel alone.
unit() {
    t=$1; f=$2; shift 2
    fmt=$(printf '%s\n' "$f" "$@" | sed -n 's/^PKT=//p; s/^convert@//p')
    src=$tmp/$t/psk_soft_amd/csrc
    if [ -z "$fmt" ]; then
        [ -f $src/$f ] && echo "$f $*"
    elif [ -f $src/psk_pkt.hip ]; then
        id=$(sed -n "s/^#define PSK_PKT_ID_$fmt //p" $src/psk_plan.h)
        case $f in convert@*) echo "psk_pkt.hip @convert_kernelILi${id}E" ;; *) echo "$f $*" | sed "s/PKT=$fmt/-DPSK_INST_PKT=$fmt/" ;; esac
    elif grep -q "PSK_INST_${fmt^^}" $src/psk_wave.h; then
        case $f in convert@*) echo "psk_$fmt.hip @convert_kernel" ;; *) echo "$f $*" | sed "s/PKT=$fmt/-DPSK_INST_${fmt^^}=1/" ;; esac
    fi
}
# build TAG TREE unit... -> $tmp/s/TAG.TREE.s (the lines of the one kernel @regex names, where given)
build() {
    tag=$1; t=$2; f=$3; shift 3
    k=$(printf '%s\n' "$@" | sed -n 's/^@//p')
    /opt/rocm/bin/hipcc $FL -I$tmp/$t/include -I$tmp/$t/psk_soft_amd/csrc $(printf '%s\n' "$@" | grep -v '^@') -o $tmp/s/$tag.$t.s \
        $tmp/$t/psk_soft_amd/csrc/$f 2>$tmp/s/$tag.$t.err || return 1
    [ -z "$k" ] || sed -i -n "/^_Z[A-Za-z0-9_]*$k[A-Za-z0-9_]*:/,/^\.Lfunc_end/p" $tmp/s/$tag.$t.s
}
one() {  # one TAG FILE [defines...]
    tag=$1; shift
    old=$(unit old "$@"); new=$(unit new "$@")
    [ -n "$new" ] || { echo "$tag: failed (no such unit in the working tree)"; return 0; }
    if [ -z "$old" ]; then
        build $tag new $new || { echo "$tag: compile failed (new): $(grep -m1 error $tmp/s/$tag.new.err)"; return 0; }
        echo "$tag: new ($(strip $tmp/s/$tag.new.s | wc -l) instructions)"
        rm -f $tmp/s/$tag.new.s
        return 0
    fi
    build $tag old $old || { echo "$tag: compile failed (old): $(grep -m1 error $tmp/s/$tag.old.err)"; return 0; }
    build $tag new $new || { echo "$tag: compile failed (new): $(grep -m1 error $tmp/s/$tag.new.err)"; return 0; }
    if cmp -s <(strip $tmp/s/$tag.old.s) <(strip $tmp/s/$tag.new.s); then
        echo "$tag: same ($(strip $tmp/s/$tag.new.s | wc -l) instructions)"
    else
        echo "$tag: DIFFERENT"
    fi
    rm -f $tmp/s/$tag.old.s $tmp/s/$tag.new.s
}
export -f unit build
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
    echo "farfit psk_farfit.hip"
    echo "tune psk_tune.hip"
    echo "resample psk_resample.hip"
    echo "fir psk_fir.hip"
    echo "acquire psk_acquire.hip"
    echo "gather psk_gather.hip"
    echo "pkt psk_pkt.hip"
    for s in $(seq 2 16); do echo "tile_inst_S$s psk_tile_inst.hip -DPSK_INST_S=$s -DPSK_INST_H=1"; done
    for f in cs16 cs8 cf16; do
        for s in $(seq 2 16); do for e in 0 1; do echo "${f}_fast_S${s}_H1_E$e psk_fast_inst.hip PKT=$f -DPSK_INST_S=$s -DPSK_INST_H=1 -DPSK_INST_E=$e"; done; done
        echo "${f}_kernels psk_kernels.hip PKT=$f"
        echo "${f}_convert convert@$f"
    done
} | sed "s/ *$//" | xargs -P 8 -L 1 bash -c 'one "$@"' _ | sort > $out
echo "$(grep -c ': same' $out) same, $(grep -c ': new' $out) new, $(grep -c 'DIFFERENT' $out) different, $(grep -c 'failed' $out) failed of $(grep -c . $out)"
[ -n "${KEEP:-}" ] || rm -rf $tmp
