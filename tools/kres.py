"""Per-kernel register / spill / LDS table from hipcc's kernel-resource-usage remarks,
over the primal loop's kernel units (the Makefile's KUNITS) or the units named.

    python tools/kres.py [filter-regex] [--units spx_price,spx_update]
"""
import argparse
import concurrent.futures
import re
import subprocess

ROOT = __file__.rsplit("/tools/", 1)[0]
ap = argparse.ArgumentParser()
ap.add_argument("filter", nargs="?")
ap.add_argument("--units", help="comma-separated unit names (default: the Makefile's KUNITS)")
args = ap.parse_args()
units = args.units.split(",") if args.units else re.search(r"^KUNITS\s*:=\s*(.*)$", open(f"{ROOT}/Makefile").read(),
                                                           re.M).group(1).split()


def remarks(unit):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", "-c",
           f"{ROOT}/simplex_method_gpu_amd/csrc/{unit}.hip", "-o", f"/tmp/kres_{unit}.o",
           "-Rpass-analysis=kernel-resource-usage"]
    return subprocess.run(cmd, capture_output=True, text=True).stderr


with concurrent.futures.ThreadPoolExecutor(len(units)) as ex:
    err = "\n".join(ex.map(remarks, units))
rows, cur = [], None
for ln in err.splitlines():
    m = re.search(r"(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                  r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+) \[-Rpass", ln)
    if not m:
        continue
    k, v = m.group(1), m.group(2)
    if k == "Function Name":
        cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
        rows.append(cur)
    elif cur is not None:
        cur[k.split(" [")[0]] = v
flt = re.compile(args.filter) if args.filter else None
for r in rows:
    if flt and not flt.search(r["name"]):
        continue
    print(f"{r['name'][:70]:70s} vgpr={r.get('VGPRs')} agpr={r.get('AGPRs')} occ={r.get('Occupancy')} "
          f"spillV={r.get('VGPRs Spill')} spillS={r.get('SGPRs Spill')} scratch={r.get('ScratchSize')}")
