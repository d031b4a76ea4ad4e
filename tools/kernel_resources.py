#!/usr/bin/env python3
"""Static resource usage of every device kernel of the library, from the compiler's own remarks
(hipcc -Rpass-analysis=kernel-resource-usage; no GPU needed): VGPRs, SGPRs, spills, scratch, LDS, occupancy per kernel, stamped with the
build id of the sources, and with the sha256 of each kernel's code bytes (two outputs with equal hashes compile identically) -- the baseline a kernel change is compared with before it goes to the GPU (round 5: the lean form of
graph_search_kernel was found by its spilled SGPRs).
    python tools/kernel_resources.py [-j 8] [-o profiles/r5_kernel_resources.json]"""
import argparse
import hashlib
import importlib.util
import json
import re
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"

spec = importlib.util.spec_from_file_location("hnsw_build", ROOT / "hnswindex.net_amd" / "build.py")
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
          "LDS Size [bytes/block]": "lds_bytes_per_block"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", o).replace("void ", "") for o in out[:len(names)]]


def code_hashes(co):
    """mangled name -> sha256 of the function's bytes in .text, from a code object (ELF64): the symbol's value and size."""
    blob = Path(co).read_bytes()
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]  # name type flags addr off size link info align entsize
    name_at = lambda tab, o: blob[tab + o:blob.index(b"\0", tab + o)].decode()
    text = next(i for i, sec in enumerate(secs) if name_at(secs[shstrndx][4], sec[0]) == ".text")
    symtab = next(sec for sec in secs if sec[1] == 2)
    out = {}
    for o in range(symtab[4], symtab[4] + symtab[5], 24):
        st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", blob, o)
        if st_info & 15 == 2 and st_shndx == text:   # STT_FUNC in .text
            start = secs[text][4] + st_value - secs[text][3]
            out[name_at(secs[symtab[6]][4], st_name)] = hashlib.sha256(blob[start:start + st_size]).hexdigest()
    return out


def unit(u, tmp):
    name, src, defs = u
    co = Path(tmp) / (name + ".co")
    cmd = [build.hipcc(), *build.FLAGS, *defs, f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "--no-gpu-bundle-output", "-c", str(CSRC / src),
           "-o", str(co), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{name}: {r.stderr[-800:]}")
    hashes = code_hashes(co)
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            mangled = t.split(":", 1)[1].strip()
            cur = {"mangled": mangled, "unit": name, "code_sha256": hashes[mangled]}
            kernels.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            if k.strip() in FIELDS:
                cur[FIELDS[k.strip()]] = int(v)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("-o", default=str(ROOT / "profiles" / "r5_kernel_resources.json"))
    a = ap.parse_args()
    us = [u for u in build.units() if u[1].endswith(".hip")]   # the units that hold device code
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as ex:
        ks = [k for res in ex.map(lambda u: unit(u, tmp), us) for k in res]
    for k, name in zip(ks, demangle([k["mangled"] for k in ks])):
        k["kernel"] = name
        del k["mangled"]
    ks.sort(key=lambda k: (k["kernel"], k["unit"]))
    out = {"build_id": build.source_id(), "flags": build.FLAGS,
           "note": "hipcc -Rpass-analysis=kernel-resource-usage per unit of build.py's units() (static; no GPU); code_sha256: the kernel's code bytes. graph_search_kernel / graph_insert_search_kernel"
                   "<METRIC (" + ", ".join(f"{i} {n}" for i, (_, n) in enumerate(build.METRICS)) + "), NS (register sets of 64 beam entries), HASHED (visited set as an id hash "
                   "table: graphs too large for a bitset per resident wave), FORM>: form 0 plain, 1 latency variant (two waves per job), 2 lean "
                   "(launches without visited sets). SGPR spills go to VGPR lanes (v_writelane / v_readlane), not to scratch, while "
                   "scratch_bytes_per_lane is 0.",
           "kernels": ks}
    Path(a.o).write_text(json.dumps(out, indent=1))
    hot = [k for k in ks if re.search(r"graph_(search|insert_search|link|range|relink)_kernel", k["kernel"])]
    for k in hot:
        print(f"{k['kernel']:<70} vgprs {k.get('vgprs'):>3} waves/SIMD {k.get('waves_per_simd')} sgpr spills {k.get('sgpr_spills'):>3} "
              f"vgpr spills {k.get('vgpr_spills')} scratch {k.get('scratch_bytes_per_lane')} lds {k.get('lds_bytes_per_block')}")
    print(f"{len(ks)} kernels -> {a.o}", file=sys.stderr)


if __name__ == "__main__":
    main()
