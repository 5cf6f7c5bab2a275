"""CPU-only sanitizer build of the launch-shape plan
(haskoin-node_amd/csrc/hkv_launch_plan.h, the code hkv_api.cpp's verify entry
points and the launch wrappers of hkv_kernels.hip run on): tests/launch_plan.cpp
checks every field of plan_records, plan_std_chunk and std_chunk_len against a
restatement of the expressions they replaced (the split, mid-size and block
thresholds, the mid-size grid, the two batched-inversion strides, the Q-scratch
size, the standard-input path's four choices and its per-tx hash choice, the
chunk rule and the table / chain chunk loop), under AddressSanitizer and
UndefinedBehaviorSanitizer (any report aborts the run): for every n from 1 to
two resident grids plus a workgroup on four geometries (an MI355X, the same
with the suite's two chunk hooks, a small partition, one block per CU), for n
within two chunks below 0xFFFFFF00 (the 64-bit chunk stepping), and at the
edges by value (4,096 / 4,097, 32,768 / 32,769, 131,072 / 131,073, 2^20 / 2^20
+ 1). Also checked: chunks are whole workgroups covering [0, n_pad) in order;
rows in kernel implies scan in kernel implies the block kernel; overlap implies
the mid-size form; the Q scratch never falls below the resident grid's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_equals_the_stepping_it_replaced_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "launch_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "launch_plan.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    # 2 * 262,144 + 256 (twice), 2 * 32,768 + 256 and 2 * 65,536 + 256 batch sizes at least
    assert int(r.stdout.split()[1]) > 1245000
