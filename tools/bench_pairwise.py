"""Measurement of the pairwise radial (Lennard-Jones) kernels (csrc/dzo_pairwise.hip) on the device: recorded, not gated.

    python tools/bench_pairwise.py [--out profiles/pairwise_bench.json] [--launches 21] [--quick]

For N in {38, 1000, 4096, 20000, 100000} and both element types:
  * kernel time of dzo_pairwise_energy / _gradient / _hvp from the library's HIP-event table (dzo_profile_*: events on the
    launching stream around the entry's kernels; warm; median of `launches` single launches), pair interactions per
    second (N^2 per call);
  * dzo_calibrate_fma_rate for the element type (register-only independent fma chains: the vector-ALU issue ceiling);
  * VALU instructions per pair in the inner loop of each kernel, counted in the disassembly of the built library (the
    smallest backward-branch loop that holds a v_rcp; VALU lines over v_rcp lines);
  * from those, pairs/s x VALU/pair over the calibrated fma issue rate (lane-instructions per second).
Alongside: the numpy fp64 twin (tests/pairwise_twin.py) on the host for N = 4096 -- the only CPU comparison there is -- and
step!()/s of L-BFGS m = 10 on the N = 4096 lattice from the problem handle against the same optimizer driven through host
callbacks (d2h, numpy twin, h2d per evaluation), which is what a user had before this objective existed on the device.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import shutil
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NS = [38, 1000, 4096, 20000, 100000]
ENTRIES = ["energy", "gradient", "hvp"]
LLVM = "/opt/rocm/lib/llvm/bin"


def valu_per_pair(lib_path):
    """{kernel name fragment: VALU instructions per pair in the inner loop} from the gfx950 code objects of the library."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        return {}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f], cwd=tmp, check=True, capture_output=True, text=True).stdout
            name, base, body = None, 0, []
            kernels = {}
            for line in text.splitlines():
                m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
                if m:
                    base, name = int(m.group(1), 16), m.group(2)
                    kernels[name] = (base, [])
                    continue
                m = re.match(r"^\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):", line)
                if m and name:
                    kernels[name][1].append((int(m.group(2), 16), m.group(1), line))
            for name, (base, ins) in kernels.items():
                m = re.search(r"pairwise_(tile|wave)_kernelI([df])NS_8LJRadialI[df]EELi([012])E", name)
                if not m:
                    continue
                addr_index = {a: k for k, (a, _, _) in enumerate(ins)}
                best = None
                for k, (a, op, line) in enumerate(ins):
                    if not op.startswith(("s_cbranch", "s_branch")):
                        continue
                    t = re.search(r"\+0x([0-9a-f]+)>", line)
                    if not t:
                        continue
                    target = base + int(t.group(1), 16)
                    if target >= a or target not in addr_index:
                        continue
                    loop = ins[addr_index[target]:k + 1]
                    rcp = sum(1 for _, o, _ in loop if o.startswith("v_rcp_f"))
                    if rcp and (best is None or len(loop) < len(best[0])):
                        best = (loop, rcp)
                if best:
                    loop, rcp = best
                    valu = sum(1 for _, o, _ in loop if o.startswith("v_"))
                    key = f"{m.group(1)}_{ENTRIES[int(m.group(3))]}_{'f64' if m.group(2) == 'd' else 'f32'}"
                    out[key] = {"valu_per_pair": valu / rcp, "pairs_per_trip": rcp, "loop_instructions": len(loop),
                                "lds_reads": sum(1 for _, o, _ in loop if o.startswith("ds_read")),
                                "global_loads": sum(1 for _, o, _ in loop if o.startswith("global_load"))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_bench.json"))
    ap.add_argument("--launches", type=int, default=21)
    ap.add_argument("--quick", action="store_true", help="N up to 4096, no optimizer / host legs (a rehearsal)")
    ap.add_argument("--ns", default=None, help="comma-separated particle counts instead of the default list (threshold sweeps)")
    ap.add_argument("--isa-only", action="store_true", help="only the instruction counts (needs no device)")
    args = ap.parse_args()

    from dzo_loader import dzo
    isa = valu_per_pair(dzo.build())
    if args.isa_only:
        print(json.dumps(isa, indent=1))
        return
    import pairwise_twin as tw
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    res = {"device": dzo.device_info(), "launches": args.launches, "wave_max_env": os.environ.get("DZO_TUNE_PAIRWISE_WAVE_MAX"),
           "note": "every number here is new: nothing in the parent commit computes this objective", "isa": isa, "fma_gflops": {}, "kernels": []}
    for dtype, tag in ((np.float64, "f64"), (np.float32, "f32")):
        rates = [dzo.calibrate_fma_rate(dtype, 1 << 16) for _ in range(5)]
        res["fma_gflops"][tag] = {"median": statistics.median(rates), "max": max(rates)}
    dzo.profile_enable(2)
    for dtype, tag in ((np.float64, "f64"), (np.float32, "f32")):
        issue_rate = res["fma_gflops"][tag]["median"] * 1e9 / 2.0            # lane-instructions per second
        for n in ([int(t) for t in args.ns.split(",")] if args.ns else (NS[:3] if args.quick else NS)):
            xyz = tw.lattice(n, seed=n)
            uvw = np.random.default_rng(n).normal(size=(3, n))
            buf = dzo.DeviceArray.from_host(np.concatenate([*xyz, *uvw]), dtype=dtype)
            x, y, z, u, v, w = (buf.view(k * n, n) for k in range(6))
            ob = dzo.DeviceArray.zeros(3 * n, dtype)
            o = [ob.view(k * n, n) for k in range(3)]
            calls = {"energy": lambda: dzo.pairwise_radial_energy(x, y, z),
                     "gradient": lambda: dzo.pairwise_radial_gradient_(*o, x, y, z),
                     "hvp": lambda: dzo.pairwise_radial_hvp_(*o, x, y, z, u, v, w)}
            for entry in ENTRIES:
                for _ in range(3):
                    calls[entry]()
                ms = []
                for _ in range(args.launches):
                    dzo.profile_reset()
                    calls[entry]()
                    ms.append(dzo.profile_table()["pairwise_" + entry][1])
                med = statistics.median(ms)
                shape = "wave" if n <= int(os.environ.get("DZO_TUNE_PAIRWISE_WAVE_MAX", "2048")) else "tile"
                k = isa.get(f"{shape}_{entry}_{tag}", {}).get("valu_per_pair")
                row = {"dtype": tag, "n": n, "entry": entry, "shape": shape, "kernel_ms_median": med, "kernel_ms_min": min(ms),
                       "kernel_ms_max": max(ms), "pairs_per_s": n * n / (med * 1e-3), "valu_per_pair": k,
                       "fraction_of_fma_issue_rate": (n * n / (med * 1e-3)) * k / issue_rate if k else None}
                res["kernels"].append(row)
                print(json.dumps(row), flush=True)
    dzo.profile_enable(0)
    if not args.quick:
        n = 4096
        xyz = tw.lattice(n, seed=1)
        p0 = np.concatenate(xyz)
        t0 = time.perf_counter(); tw.energy_f64(p0); t1 = time.perf_counter(); tw.gradient_f64(p0); t2 = time.perf_counter()
        res["host_numpy_fp64_n4096"] = {"energy_s": t1 - t0, "gradient_s": t2 - t1, "threads": os.environ.get("OMP_NUM_THREADS"),
                                        "label": "numpy twin on the host CPU, the only CPU comparison available"}
        prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
        opt = dzo.LBFGSOptimizer(None, prob, None, dzo.DeviceArray.from_host(p0), 0.01, 10)
        for _ in range(5):
            opt.step()
        dzo.synchronize()
        t0 = time.perf_counter()
        for _ in range(40):
            opt.step()
        dzo.synchronize()
        dev_rate = 40 / (time.perf_counter() - t0)

        def f_host(x):
            return tw.energy_f64(x.to_host())

        def g_host(g, x):
            g.upload(tw.gradient_f64(x.to_host()))
        opt_h = dzo.LBFGSOptimizer(None, f_host, g_host, dzo.DeviceArray.from_host(p0), 0.01, 10)
        t0 = time.perf_counter()
        for _ in range(3):
            opt_h.step()
        dzo.synchronize()
        host_rate = 3 / (time.perf_counter() - t0)
        res["lbfgs_m10_n4096_steps_per_s"] = {"problem_handle": dev_rate, "host_callbacks_numpy": host_rate,
                                              "f_after": opt.current_objective_value}
        print(json.dumps(res["lbfgs_m10_n4096_steps_per_s"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
