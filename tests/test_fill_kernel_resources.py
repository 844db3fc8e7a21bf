"""CPU-side checks of the fill kernel's two-windows-per-CU instantiation: the LDS layout's static_asserts compile, and the cross-compiled kernel's
resource report leaves room for two 512-thread workgroups on one CU (four waves per SIMD: at most 128 VGPRs, no scratch).  No GPU needed; the
launch site checks the same occupancy on the device."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mir-prefer_amd", "csrc")
NEW_KERNEL = "fold_lds_kernelILi0ELb1ELi512EE"      # mirp::fold_lds_kernel<0, true, 512>


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_two_per_cu_instantiation_fits_two_workgroups(tmp_path):
    cmd = [_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "fold_lds_kernel.hip"), "-o", str(tmp_path / "fold_lds_kernel.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]      # includes the layout static_asserts of fold_lds_common.h
    report = {}
    name = None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    new = [v for k, v in report.items() if NEW_KERNEL in k]
    assert len(new) == 1, sorted(report)
    r = new[0]
    print("fold_lds_kernel<0, true, 512>:", r)
    assert r["VGPRs"] <= 128, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= 4, r      # waves per SIMD: 2 workgroups x 8 waves on 4 SIMDs
    assert r["LDS Size"] == 0, r       # no static LDS beside the dynamic 80 KB the launch asks for
    # the 1024-thread candidate-pool instantiation of the default model is gone from the product: only the dense pass and vienna-1.8.5 keep that geometry
    assert not [k for k in report if "fold_lds_kernelILi0ELb1ELi1024EE" in k]
