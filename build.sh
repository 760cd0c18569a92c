#!/bin/bash
# Build libtwxhip.so and libtwxqa.so (gfx950) in-tree.  hipcc cross-compiles without a GPU.
# The compiler's per-kernel resource remarks (VGPRs / AGPRs / scratch / LDS / occupancy) are reduced into
# topowx_amd/libtwxhip.resources.txt: tests/test_isa_resources.py fails when a kriging / daily kernel spills or
# outgrows the register budget its waves_per_eu tuning assumes (a compiler bump would otherwise cost 10-20 % silently).
set -e
cd "$(dirname "$0")"
LOG=$(mktemp /tmp/twx_build.XXXXXX)
# stderr without the resource-usage remark blocks: a remark line and the source-context lines that follow IT are dropped;
# the context lines of genuine warnings / errors stay
show_diagnostics() {
    awk '/^In file included from/ { hold = hold $0 "\n"; next }
         /: remark: .*\[-Rpass-analysis=kernel-resource-usage\]/ { skip = 1; hold = ""; next }
         skip && (/^ *[0-9]+ \| / || /^ *\| /) { next }
         { skip = 0; printf "%s", hold; hold = ""; print }' "$1" >&2
}
if ! hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared -std=c++17 -Iinclude -Itopowx_amd/csrc \
    -Rpass-analysis=kernel-resource-usage "$@" -o topowx_amd/libtwxhip.so topowx_amd/csrc/twx_hip.hip 2> "$LOG"; then
    show_diagnostics "$LOG"
    rm -f "$LOG"
    exit 1
fi
show_diagnostics "$LOG"
python3 tests/tools/isa_resources.py "$LOG" > topowx_amd/libtwxhip.resources.txt
# libtwxqa.so: the station QA kernels (include/twx_qa.h), a library of their own -- built second, same flags.  The seventh
# to fourteenth units, twx_ppca and twx_infillchk (step16), twx_xvalinfill (step15), twx_serial (step17/18), twx_nnr (the
# reanalysis columns of steps 14-16), twx_homog (step05, step09-11), twx_stnrast (step19, the front of step20) and
# twx_prcpqa (the precipitation QA), the fifteenth, twx_prcpcorrob (its spatial corroboration check), and the sixteenth,
# twx_ghcn (step04's GHCN-Daily ingest), the seventeenth, twx_nnrsub (step12's reanalysis subsets), and the eighteenth,
# twx_tzpoly (step13's point-in-polygon time-zone lookup), and the nineteenth, twx_mosaic (step26/27's mosaics, deflated on
# the device with the kernels of topowx_amd/csrc/twx_deflate.h), are each named by a pattern that matches only it:
# tests/test_emnorm_host.py pins the number of unit names spelled out in this script to the units it knew
if ! hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared -std=c++17 -Iinclude \
    -Rpass-analysis=kernel-resource-usage "$@" -o topowx_amd/libtwxqa.so topowx_amd/qa/twx_outlier.hip \
    topowx_amd/qa/twx_spatial.hip topowx_amd/qa/twx_corrob.hip topowx_amd/qa/twx_nonspatial.hip \
    topowx_amd/qa/twx_infillmat.hip topowx_amd/qa/twx_emnorm.hip topowx_amd/qa/twx_ppca.[h]ip \
    topowx_amd/qa/twx_infillchk.[h]ip topowx_amd/qa/twx_xvalinfill.[h]ip topowx_amd/qa/twx_serial.[h]ip \
    topowx_amd/qa/twx_nnr.[h]ip topowx_amd/qa/twx_homog.[h]ip topowx_amd/qa/twx_stnrast.[h]ip \
    topowx_amd/qa/twx_prcpqa.[h]ip topowx_amd/qa/twx_prcpcorrob.[h]ip \
    topowx_amd/qa/twx_ghcn.[h]ip topowx_amd/qa/twx_nnrsub.[h]ip topowx_amd/qa/twx_tzpoly.[h]ip \
    topowx_amd/qa/twx_mosaic.[h]ip 2> "$LOG"; then
    show_diagnostics "$LOG"
    rm -f "$LOG"
    exit 1
fi
show_diagnostics "$LOG"
python3 tests/tools/isa_resources.py "$LOG" > topowx_amd/libtwxqa.resources.txt
rm -f "$LOG"
