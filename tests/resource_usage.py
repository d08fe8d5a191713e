"""What hipcc reports per kernel under -Rpass-analysis=kernel-resource-usage, for the tests that pin register and LDS figures of the stretch kernels."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size"]


def parse(remarks):
    """{mangled kernel name: {field: value}} from the compiler's remark text."""
    kernels, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels


def resources(source):
    """Compiles phaze_amd/csrc/<source> for gfx950 with the product's optimisation flags (device side only) and returns parse() of its remarks."""
    src = os.path.join(ROOT, "phaze_amd", "csrc")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", os.devnull, source], cwd=src, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return parse(out.stderr)


def stretch_key(name):
    """A mangled name of pv_stretch_kernels.hip or pv_onset_kernels.hip as a readable key: ("a" | "b", log2n, SCHED, LINK, RESET) for a pass,
    ("scan", "stretch" | "reset") for a scan, ("onset", log2n) for the onset-strength kernel; None for anything else."""
    m = re.search(r"pv_stretch_pass_([ab])ILi(\d+)ELb([01])ELb([01])ELb([01])E", name)
    if m:
        return (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
    m = re.search(r"\d+pv_(stretch|reset)_scanE", name)
    if m:
        return ("scan", m.group(1))
    m = re.search(r"pv_onset_strength_kernelILi(\d+)E", name)
    if m:
        return ("onset", int(m.group(1)))
    return None
