#!/bin/bash
# What keeps the row-prefilter search kernels (graph_search_kernel<M_SQ, NS, HASHED, form 3 / 4>) from four waves per
# SIMD?  Static experiment, no GPU and no change to the product: the search_lean unit of sq_euclid is compiled as shipped, with the
# run-time-length form pinned to four waves (-DHNSW_PF_WAVES=4), with the fixed-length form pinned to three (-DHNSW_PF_FIXED_WAVES=3),
# and -- in a scratch copy of csrc/ in which search_job returns before the exact two-heap traversal in the prefilter forms
# (-DEXP_PF_NO_EXACT) -- at four waves without that traversal.  The compiler's resource remarks (hipcc
# -Rpass-analysis=kernel-resource-usage) are printed per build.  Form 3 reads the row length at run time, form 4 has it compiled in.
#   usage: tools/pf_fixed_dim_static.sh > profiles/pf_fixed_dim_static.txt
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
mkdir -p $T/pkg/x && cp -r $R/hnswindex.net_amd/csrc $T/pkg/x/csrc && cp -r $R/include $T/pkg/include   # csrc includes ../../include/...
cd $T/pkg/x/csrc
python3 - <<'E'
f = "dk_search_kernels.h"
s = open(f).read()
at = "    bool aborted = false;\n    bool ok;\n    if constexpr (LEAN) {\n"
assert s.count(at) == 1
s = s.replace(at, "#ifdef EXP_PF_NO_EXACT\n    if constexpr (form_is_pf(FORM)) return;\n#endif\n" + at)
open(f, "w").write(s)
E
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -I. --cuda-device-only"
UNIT="-DHNSW_UNIT_KIND=search_lean -DHNSW_UNIT_METRIC=sq kernel_unit.hip"
compile() { # tag, extra flags
  local tag=$1; shift
  hipcc $FLAGS "$@" -c $UNIT -o $T/$tag.o -Rpass-analysis=kernel-resource-usage 2> $T/$tag.txt
}
report() { # tag, title
  python3 - $T/$1.txt "$2" <<'E'
import re, subprocess, sys
txt, title = sys.argv[1:3]
rows, cur = [], None
for line in open(txt):
    m = re.search(r"remark:\s*(.*?)\s*\[-Rpass-analysis", line)
    if not m:
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        name = subprocess.run(["c++filt", t.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
        cur = {"k": re.sub(r"\(.*", "", name).replace("void hnsw::", "")}
        rows.append(cur)
    elif cur is not None and ":" in t:
        k, v = t.rsplit(":", 1)
        cur[k.strip()] = v.strip()
print(f"== {title}")
for r in rows:
    if not re.search(r"graph_search_kernel<0, \d, (true|false), [34]>", r["k"]):
        continue
    print(f"   {r['k']:<44} VGPRs {r.get('VGPRs'):>3}  spilled VGPRs {r.get('VGPRs Spill'):>2}  scratch {r.get('ScratchSize [bytes/lane]'):>3} B/lane  "
          f"spilled SGPRs {r.get('SGPRs Spill'):>3}  waves/SIMD {r.get('Occupancy [waves/SIMD]')}")
E
}
echo "# tools/pf_fixed_dim_static.sh: the row-prefilter search kernels of sq_euclid (unit search_lean_sq), static, no GPU"
echo "# graph_search_kernel<METRIC 0 = sq_euclid, NS register sets, HASHED, FORM>: form 3 = row length read at run time, form 4 = row length 128 compiled in"
compile a &
compile b -DHNSW_PF_WAVES=4 &
compile c -DHNSW_PF_WAVES=4 -DEXP_PF_NO_EXACT &
compile d -DHNSW_PF_FIXED_WAVES=3 &
wait
report a "as shipped: form 3 at three waves per SIMD, form 4 at four"
report b "-DHNSW_PF_WAVES=4: form 3 at four waves as well"
report c "-DHNSW_PF_WAVES=4 -DEXP_PF_NO_EXACT: both forms at four waves, the exact two-heap re-run compiled out of them"
report d "-DHNSW_PF_FIXED_WAVES=3: form 4 at three waves"
