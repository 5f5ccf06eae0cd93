#!/usr/bin/env python3
"""tools/device_forms_probe.py -- what dasp_plan_create_device costs on the matrices that take the two-phase form or column-blocked long rows, with the
device packers of those forms (r8) against a library that fetches the CSR and packs them on the host (the parent revision, built with tools/build_rev.sh).

One process per library (a library is chosen at import: DASP_AMD_SO), one JSON file per process:

    python tools/device_forms_probe.py --run new.json                              # this tree's library
    DASP_AMD_SO=dasp_amd/variants/parent/libdasp_amd.so python tools/device_forms_probe.py --run parent.json
    python tools/device_forms_probe.py --laps laps.txt                              # DASP_VERBOSE=1 laps of one build per input (this tree's library)
    python tools/device_forms_probe.py --report profiles/r08_device_forms.md parent1.json new1.json parent2.json new2.json [--laps-file laps.txt]

--run: per input (values all ones, CSR resident on the device) one untimed build (code object and hipcub loads), then three timed ones: host clock around
dasp_plan_create_device, device synchronised before and after; peak extra device memory = the largest drop of hipMemGetInfo's free bytes seen by a sampler
thread during the first timed build, minus what the finished plan keeps.
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = (("ljournal-2008", 16), ("rmat_2M", 16), ("powerlaw_1M", 16), ("powerlaw_1M", 64), ("ljournal-2008-uniform", 16))
QUOTED = "VERDICT r6 asked for ljournal-2008 f16 <= 40 ms from a device CSR; README (r6) recorded 0.3-0.4 s of fetch plus 0.15-0.2 s of host packing for ljournal-2008 / powerlaw_1M."


def device_csr(D, torch, name, prec):
    rows, cols = D.synth_dims(name, 1.0)
    rp, ci = D.synth_csr(name, 1.0)
    nnz = int(rp[-1])
    d_rp, d_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    d_v = torch.ones(nnz, dtype=torch.float64 if prec == 64 else torch.float16, device="cuda")
    return rows, cols, nnz, d_rp, d_ci, d_v


def build(D, torch, csr, prec):
    rows, cols, nnz, d_rp, d_ci, d_v = csr
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = D.Plan.from_device(d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), rows, cols, nnz, precision=prec)
    torch.cuda.synchronize()
    return p, (time.perf_counter() - t0) * 1e3


def run(out):
    import torch
    import dasp_amd as D
    torch.cuda.set_device(0)
    res = dict(library=os.environ.get("DASP_AMD_SO", D.SO_PATH), inputs=[])
    for name, prec in INPUTS:
        csr = device_csr(D, torch, name, prec)
        p, _ = build(D, torch, csr, prec)          # untimed
        p.close()
        times, peak, kept, fetched, st = [], 0, 0, None, {}
        for k in range(3):
            free0 = torch.cuda.mem_get_info()[0]
            low, stop = [free0], threading.Event()

            def sample():
                while not stop.is_set():
                    low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                    time.sleep(0.0005)
            th = threading.Thread(target=sample) if k == 0 else None
            if th:
                th.start()
            p, ms = build(D, torch, csr, prec)
            if th:
                stop.set()
                th.join()
                kept = free0 - torch.cuda.mem_get_info()[0]
                peak = max(0, free0 - low[0] - kept)
            times.append(ms)
            st = p.stats
            try:
                fetched = p.csr_fetch_bytes
            except AttributeError:
                fetched = None                     # (a library without the counter)
            p.close()
        res["inputs"].append(dict(name=name, prec=prec, nnz=csr[2], ms=times, peak_extra_bytes=int(peak), plan_bytes=int(kept), csr_fetch_bytes=fetched,
                                  two_phase=st.get("two_phase"), tp_segments=st.get("tp_segments"), lcb_rows=st.get("lcb_rows"), n_col_panels=st.get("n_col_panels")))
        print("%-24s f%-2d %s ms  peak extra %.2f GB  fetched %s" % (name, prec, " ".join("%.1f" % t for t in times), peak / 1e9, fetched), flush=True)
        del csr
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def laps(out):
    """one build per input in a child process each, DASP_VERBOSE=1, stderr kept"""
    import subprocess
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport dasp_amd as D, device_forms_probe as P\n"
            "csr = P.device_csr(D, torch, sys.argv[1], int(sys.argv[2])); p, ms = P.build(D, torch, csr, int(sys.argv[2])); p.close()\n"
            "import os; os.environ['DASP_VERBOSE'] = '1'\np, ms = P.build(D, torch, csr, int(sys.argv[2])); print('== %%s f%%s: %%.1f ms' %% (sys.argv[1], sys.argv[2], ms))\n"
            % (ROOT, os.path.join(ROOT, "tools")))
    with open(out, "w") as f:
        for name, prec in INPUTS:
            r = subprocess.run([sys.executable, "-c", code, name, str(prec)], capture_output=True, text=True, timeout=600)
            f.write("### %s f%d\n%s%s\n" % (name, prec, r.stderr, r.stdout))
            f.flush()
            if r.returncode != 0:
                raise SystemExit("laps of %s f%d failed (%d)" % (name, prec, r.returncode))


def report(out, files, laps_file):
    runs = [json.load(open(f)) for f in files]
    is_parent = lambda r: "variants" in r["library"]
    lines = ["# dasp_plan_create_device on the two-phase / hub-row matrices: device packers (r8) against the fetch-and-host-pack of the parent revision", "",
             "`tools/device_forms_probe.py`: values all ones, CSR resident on the device, wall ms of `dasp_plan_create_device` (device synchronised before and after);",
             "one process per library, alternating parent / new, one untimed build first in each process, then three timed ones.", "",
             "| input | prec | nnz | parent ms (all runs) | new ms (all runs) | fastest parent | slowest new | slowest new < fastest parent | peak extra device memory (new) | B / nnz | fetched (parent -> new) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    ok_all = True
    for i, (name, prec) in enumerate(INPUTS):
        par = [t for r in runs if is_parent(r) for t in r["inputs"][i]["ms"]]
        new = [t for r in runs if not is_parent(r) for t in r["inputs"][i]["ms"]]
        first_new = [r for r in runs if not is_parent(r)][0]["inputs"][i]
        ok = bool(par) and bool(new) and max(new) < min(par)
        ok_all = ok_all and ok
        lines.append("| %s | f%d | %d | %s | %s | %.1f | %.1f | %s | %.2f GB | %.1f | %s -> %s |" % (
            name, prec, first_new["nnz"], " ".join("%.1f" % t for t in par), " ".join("%.1f" % t for t in new), min(par) if par else -1, max(new) if new else -1,
            "yes" if ok else "NO", first_new["peak_extra_bytes"] / 1e9, first_new["peak_extra_bytes"] / max(1, first_new["nnz"]),
            "n/a (no counter)", first_new["csr_fetch_bytes"]))
    lines += ["", "Requirement (every input: the slowest timed build of the new library is faster than the fastest of the parent's): %s." % ("met" if ok_all else "NOT met"), "",
              QUOTED, ""]
    lj = [t for r in runs if not is_parent(r) for t in r["inputs"][0]["ms"]]
    if lj:
        lines.append("ljournal-2008 f16 with the device packers: %.1f-%.1f ms -- the 40 ms of VERDICT r6 are %s." % (min(lj), max(lj), "reached" if max(lj) <= 40 else "not reached"))
    if laps_file and os.path.exists(laps_file):
        lines += ["", "## DASP_VERBOSE=1 laps of one build per input (new library)", "", "```", open(laps_file).read().rstrip(), "```"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out, "requirement", "met" if ok_all else "NOT met")


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
