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
# libtwxqa.so: the station QA kernels (include/twx_qa.h), a library of their own -- built second, same flags.  Every unit
# of topowx_amd/qa is named here once (tests/test_emnorm_host.py compares the names with the directory; twxrw_raws.hip is
# checked by tests/test_raws_host.py and stays last, twxsd_serdeflate.hip by tests/test_series_deflate_host.py); the headers next to them (twx_qa_common.h, twx_qa_series.h, ...) are no units;
# twx_mosaic deflates with the kernels of topowx_amd/csrc/twx_deflate.h.
if ! hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared -std=c++17 -Iinclude \
    -Rpass-analysis=kernel-resource-usage "$@" -o topowx_amd/libtwxqa.so topowx_amd/qa/twx_outlier.hip \
    topowx_amd/qa/twx_spatial.hip topowx_amd/qa/twx_corrob.hip topowx_amd/qa/twx_nonspatial.hip \
    topowx_amd/qa/twx_infillmat.hip topowx_amd/qa/twx_emnorm.hip topowx_amd/qa/twx_ppca.hip \
    topowx_amd/qa/twx_infillchk.hip topowx_amd/qa/twx_xvalinfill.hip topowx_amd/qa/twx_serial.hip \
    topowx_amd/qa/twx_nnr.hip topowx_amd/qa/twx_homog.hip topowx_amd/qa/twx_stnrast.hip \
    topowx_amd/qa/twx_prcpqa.hip topowx_amd/qa/twx_prcpcorrob.hip \
    topowx_amd/qa/twx_ghcn.hip topowx_amd/qa/twx_nnrsub.hip topowx_amd/qa/twx_tzpoly.hip \
    topowx_amd/qa/twx_mosaic.hip topowx_amd/qa/twxsd_serdeflate.hip topowx_amd/qa/twxrw_raws.hip 2> "$LOG"; then
    show_diagnostics "$LOG"
    rm -f "$LOG"
    exit 1
fi
show_diagnostics "$LOG"
python3 tests/tools/isa_resources.py "$LOG" > topowx_amd/libtwxqa.resources.txt
rm -f "$LOG"
