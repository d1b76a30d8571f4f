"""Generator of tests/golden/optim_bits.json: sha256 digests of every stream the fused optimizer writes -- parameters, moments, max_exp_avg_sq, the
weight average, the bf16 compute copies, the step counter, the control block -- after every step of the cases of tests/optim_bits_cases.py, on the GPU.

    python tests/golden/make_optim_bits_golden.py --parent <hash of the checked-out commit> [--out tests/golden/optim_bits.json]

Run it from a checkout of a commit whose optimizer is KNOWN TO BE GOOD, built for gfx950 -- never from the code that tests/test_gpu_optim_bits.py is
about to judge.  The file in the repository was recorded from f2f7231, the last commit before the optimizer's kernels were gathered in csrc/optim.hip.

The kernels are free of atomics and documented as bit-reproducible, so every case is run twice and nothing is written unless both runs agree digest
for digest.  The digests depend on the code the compiler generates for powf / rsqrtf / the division: the file also records the `hipcc --version` line.
If a later toolchain changes that code generation, the test fails on every case at once although no source changed; the fixture is then regenerated
with this script from a commit known to be good under the new toolchain."""
import argparse
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def hipcc_version():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    text = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
    return next((ln.strip() for ln in text.split("\n") if ln.startswith("HIP version")), text.split("\n")[0].strip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit this checkout is at")
    ap.add_argument("--out", default=os.path.join(HERE, "optim_bits.json"))
    args = ap.parse_args()
    import optim_bits_cases as C
    runs = [{name: C.run_case(name) for name in C.CASES} for _ in range(2)]
    for name in C.CASES:
        differ = [k for k in runs[0][name] if runs[0][name][k] != runs[1][name].get(k)]
        if differ or list(runs[0][name]) != list(runs[1][name]):
            sys.exit(f"case {name}: two runs of the same code differ at {differ[:8]}: nothing written")
    with open(args.out, "w") as f:
        json.dump({"parent": args.parent, "hipcc": hipcc_version(), "cases": runs[0]}, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"wrote {args.out}: {len(C.CASES)} cases, {sum(len(v) for v in runs[0].values())} digests")


if __name__ == "__main__":
    main()
