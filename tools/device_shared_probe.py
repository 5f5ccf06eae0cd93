#!/usr/bin/env python3
"""tools/device_shared_probe.py -- what deriving the shared id plane on the GPU costs and gives a plan built by dasp_plan_create_device (r17), on the f64 plans that
stream from HBM, against the parent revision (built with tools/build_rev.sh) -- the protocol of tools/device_forms_probe.py: one process per library (a library is
chosen at import: DASP_AMD_SO), alternating, one JSON file per process; no DASP_SHARE_IDS anywhere (the automatic rule decides).

    python tools/device_shared_probe.py --run new1.json                              # this tree's library
    DASP_AMD_SO=dasp_amd/variants/parent/libdasp_amd.so python tools/device_shared_probe.py --run parent1.json
    python tools/device_shared_probe.py --laps laps.txt                              # DASP_VERBOSE=1 laps of one build per input (this tree's library)
    python tools/device_shared_probe.py --report profiles/r17_device_shared_ids.md parent1.json new1.json parent2.json new2.json [--laps-file laps.txt]

--run, per input (values all ones, CSR resident on the device): one untimed build, then three timed ones (host clock around dasp_plan_create_device, device
synchronised before and after) -- and, with a library that has the derivation, three more under DASP_DEVPACK_SHARED=0; then the product: ms per SpMV (one event pair
around 200 launches, 20 warm-up) of a device-built plan, of one built under DASP_DEVPACK_SHARED=0 and of a host-built, uploaded one, each built three times, in turn.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = ("HV15R", "HV15R-unstructured", "Queen_4147")


class knob:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("DASP_DEVPACK_SHARED")
        if self.value is not None:
            os.environ["DASP_DEVPACK_SHARED"] = self.value

    def __exit__(self, *a):
        os.environ.pop("DASP_DEVPACK_SHARED", None)
        if self.old is not None:
            os.environ["DASP_DEVPACK_SHARED"] = self.old


def device_csr(D, torch, name):
    rows, cols = D.synth_dims(name, 1.0)
    rp, ci = D.synth_csr(name, 1.0)
    nnz = int(rp[-1])
    d_rp, d_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    d_v = torch.ones(nnz, dtype=torch.float64, device="cuda")
    return dict(rows=rows, cols=cols, nnz=nnz, rp=rp, ci=ci, d=(d_rp, d_ci, d_v))


def build(D, torch, csr, shared=None):
    d_rp, d_ci, d_v = csr["d"]
    with knob(shared):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = D.Plan.from_device(d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), csr["rows"], csr["cols"], csr["nnz"], precision=64)
        torch.cuda.synchronize()
    return p, (time.perf_counter() - t0) * 1e3


def facts(p):
    out = dict(kernel=p.kernel_variant())
    if hasattr(p, "shared_ids"):
        out.update(p.shared_ids())
        out["pair_mask"] = p.pair_mask()
    return out


def run(out):
    import numpy as np
    import torch
    import dasp_amd as D
    torch.cuda.set_device(0)
    lib = os.environ.get("DASP_AMD_SO", D.SO_PATH)
    parent = "variants" in lib
    res = dict(library=lib, inputs=[])
    for name in INPUTS:
        csr = device_csr(D, torch, name)
        p, _ = build(D, torch, csr)          # untimed
        p.close()
        ms, ms_off = [], []
        for shared, into in ((None, ms),) + (() if parent else (("0", ms_off),)):
            for _ in range(3):
                p, t = build(D, torch, csr, shared)
                into.append(t)
                dev_facts = facts(p) if shared is None else dev_facts
                p.close()
        x = torch.ones(csr["cols"], dtype=torch.float64, device="cuda")
        y = torch.zeros(csr["rows"], dtype=torch.float64, device="cuda")
        spmv = dict(device=[], device_off=[], host=[])
        host_facts = None
        ones = np.ones(csr["nnz"])
        for _ in range(3):
            kinds = [("device", lambda: build(D, torch, csr)[0]), ("host", lambda: D.Plan(csr["rp"], csr["ci"], ones, csr["cols"], precision=64).upload())]
            if not parent:
                kinds.insert(1, ("device_off", lambda: build(D, torch, csr, "0")[0]))
            for kind, make in kinds:
                p = make()
                spmv[kind].append(p.time(x.data_ptr(), y.data_ptr(), 0, 20, 200)[1])
                if kind == "host":
                    host_facts = facts(p)
                p.close()
        res["inputs"].append(dict(name=name, nnz=csr["nnz"], ms=ms, ms_off=ms_off, device=dev_facts, host=host_facts, spmv_ms=spmv))
        print("%-20s build %s | off %s | spmv %s" % (name, " ".join("%.1f" % t for t in ms), " ".join("%.1f" % t for t in ms_off),
                                                    {k: ["%.4f" % t for t in v] for k, v in spmv.items()}), flush=True)
        print("   device-built:", dev_facts, "\n   host-built:  ", host_facts, flush=True)
        del csr, x, y
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def laps(out):
    """one build per input in a child process each, DASP_VERBOSE=1, stderr kept"""
    import subprocess
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport dasp_amd as D, device_shared_probe as P\n"
            "csr = P.device_csr(D, torch, sys.argv[1]); p, ms = P.build(D, torch, csr); p.close()\n"
            "import os; os.environ['DASP_VERBOSE'] = '1'\np, ms = P.build(D, torch, csr); print('== %%s: %%.1f ms' %% (sys.argv[1], ms))\n"
            % (ROOT, os.path.join(ROOT, "tools")))
    with open(out, "w") as f:
        for name in INPUTS:
            r = subprocess.run([sys.executable, "-c", code, name], capture_output=True, text=True, timeout=600)
            keep = [l for l in r.stderr.splitlines() if l.startswith("[dasp shared]") or "device pack" in l]
            f.write("### %s\n%s\n%s\n" % (name, "\n".join(keep), r.stdout))
            f.flush()
            if r.returncode != 0:
                raise SystemExit("laps of %s failed (%d)\n%s" % (name, r.returncode, r.stderr[-2000:]))


def report(out, files, laps_file):
    runs = [json.load(open(f)) for f in files]
    is_parent = lambda r: "variants" in r["library"]
    new_runs, par_runs = [r for r in runs if not is_parent(r)], [r for r in runs if is_parent(r)]
    span = lambda v: "%.4f-%.4f" % (min(v), max(v)) if v else "n/a"
    L = ["# The shared id plane derived on the GPU for plans built from a device CSR (r17)", "",
         "`tools/device_shared_probe.py`: f64, full size, values all ones, CSR resident on the device, default options, no `DASP_SHARE_IDS`; one process per library,",
         "alternating parent / new, one untimed build first in each process.  The parent is the commit before this one (`tools/build_rev.sh`).", "",
         "## (a) The automatic choice: device-built against host-built plan (this commit)", "",
         "| input | nnz | host-built: in use, kernel | device-built: in use, kernel | paired id bytes / plane + table (device = host?) | pair mask set bits in use (device / host) | agree |",
         "|---|---|---|---|---|---|---|"]
    for i, name in enumerate(INPUTS):
        r = new_runs[0]["inputs"][i]
        d, h = r["device"], r["host"]
        same = all(d.get(k) == h.get(k) for k in ("available", "paired_id_bytes", "shared_bytes", "in_use", "kernel", "pair_mask"))
        L.append("| %s | %d | %s, `%s` | %s, `%s` | %d / %d (%s) | %d / %d | %s |" % (
            name, r["nnz"], h["in_use"], h["kernel"], d["in_use"], d["kernel"], d["paired_id_bytes"], d["shared_bytes"],
            "yes" if (d["paired_id_bytes"], d["shared_bytes"]) == (h["paired_id_bytes"], h["shared_bytes"]) else "NO",
            d["pair_mask"]["set_bits_in_use"], h["pair_mask"]["set_bits_in_use"], "yes" if same else "NO"))
    L += ["", "## (b) Wall ms of `dasp_plan_create_device`", "",
          "| input | parent (all runs) | this commit (all runs) | this commit, `DASP_DEVPACK_SHARED=0` | fastest parent | slowest new | slowest new - fastest parent |", "|---|---|---|---|---|---|---|"]
    for i, name in enumerate(INPUTS):
        par = [t for r in par_runs for t in r["inputs"][i]["ms"]]
        new = [t for r in new_runs for t in r["inputs"][i]["ms"]]
        off = [t for r in new_runs for t in r["inputs"][i]["ms_off"]]
        L.append("| %s | %s | %s | %s | %.1f | %.1f | %+.1f |" % (name, " ".join("%.1f" % t for t in par), " ".join("%.1f" % t for t in new), " ".join("%.1f" % t for t in off),
                                                                min(par) if par else -1, max(new) if new else -1, (max(new) - min(par)) if par and new else 0))
    L += ["", "## (c) ms per SpMV (event time over 200 launches; every plan built three times per process, in turn)", "",
          "| input | device-built, this commit | device-built, `DASP_DEVPACK_SHARED=0` | host-built, this commit | device-built, parent | host-built, parent | best device-built / best `=0` | best device-built / best host-built |",
          "|---|---|---|---|---|---|---|---|"]
    for i, name in enumerate(INPUTS):
        g = lambda rs, k: [t for r in rs for t in r["inputs"][i]["spmv_ms"].get(k, [])]
        dv, of, ho, pd, ph = g(new_runs, "device"), g(new_runs, "device_off"), g(new_runs, "host"), g(par_runs, "device"), g(par_runs, "host")
        L.append("| %s | %s | %s | %s | %s | %s | %.3f | %.3f |" % (name, span(dv), span(of), span(ho), span(pd), span(ph), min(dv) / min(of), min(dv) / min(ho)))
    if laps_file and os.path.exists(laps_file):
        L += ["", "## Inside the derivation: DASP_VERBOSE=1 laps of one build per input (this commit)", "", "```", open(laps_file).read().rstrip(), "```"]
    with open(out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--laps")
    ap.add_argument("--report")
    ap.add_argument("--laps-file", default="")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    if a.run:
        run(a.run)
    elif a.laps:
        laps(a.laps)
    elif a.report:
        report(a.report, a.files, a.laps_file)
    else:
        ap.error("one of --run, --laps, --report")


if __name__ == "__main__":
    main()
