"""The stand-alone host checks under tests/host: headers of vrenderer_amd/csrc that compile without HIP, each driven by a C++
program that prints its case count and "N failures"."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_check(tmp_path, name, extra=(), exe=None):
    """Compiles tests/host/<name>.cpp against vrenderer_amd/csrc into tmp_path/<exe or name>; returns the executable's path."""
    exe = os.path.join(str(tmp_path), exe or name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "vrenderer_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run_host_check(exe, *args, timeout=120, expect=" 0 failures", stderr_tail=2000):
    """Runs a check; it must exit 0 and print `expect`.  Returns the completed process for the caller's own counts."""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and expect in r.stdout, r.stdout[-4000:] + r.stderr[-stderr_tail:]
    return r


def build_host_example(tmpdir):
    exe = os.path.join(str(tmpdir), "frame_example")
    lib_dir = os.path.join(ROOT, "vrenderer_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "frame_example.cpp"), "-o", exe,
           "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def build_allgather_example(tmpdir):
    exe = os.path.join(str(tmpdir), "frame_allgather_example")
    lib_dir = os.path.join(ROOT, "vrenderer_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "host", "frame_allgather_example.cpp"), "-o", exe,
           "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lrccl", "-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe
