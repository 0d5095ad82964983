"""render.h's trace-instance rules on the host (no GPU): tests/trace_variant_check.cpp
states the normalisation rules, the table key's range and injectivity and the
fourteen conditions of trace_plain_ok as predicates of its own and checks
render.h against them over all 4 x 2 x 4 x 5 x 2 x 2 requests.  Built with
AddressSanitizer + UndefinedBehaviorSanitizer as tests/test_host_sanitizers.py
builds its program: render.h is plain C++ once the HIP platform is named."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_trace_variant_rules(tmp_path):
    exe = str(tmp_path / "trace_variant_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{CSRC}", f"-I{os.path.join(ROCM, 'include')}",
                    os.path.join(ROOT, "tests", "trace_variant_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    counts = dict(zip(r.stdout.split()[::2], map(int, r.stdout.split()[1::2])))
    assert counts["requests"] == 640 and counts["conditions"] == 14 and counts["failures"] == 0
    # the instances that exist: per step, 3 searches x (4 families x 5 kinds less SERIAL on the wide walk)
    # and the corner search's 4 sphere-only kinds; then the deferred-leaf instance and its plain twin
    assert counts["keys"] == 2 * (3 * 19 + 4) + 2
