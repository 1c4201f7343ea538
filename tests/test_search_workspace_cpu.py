"""The search workspaces' layouts (csrc/bg_workspace.h) on the host: a stand-alone program
(tests/cpp/workspace_main.cpp) built with AddressSanitizer + UBSan checks, over a grid of
shapes with the corner cases, that every region starts on a 256-byte boundary, that the
regions are disjoint and in declaration order, that bytes() is the end of the last one,
that the 2-ply head does not depend on the row and job counts, and three fixed sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc")


def test_workspace_layouts(tmp_path):
    exe = str(tmp_path / "workspace_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "workspace_main.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "workspace ok" in r.stdout and "runtime error" not in r.stderr
