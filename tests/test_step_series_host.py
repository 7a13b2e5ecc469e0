"""The observers' host-side series (sphexample_amd/csrc/sphmi_series.h: StepSeries, the two deliver functions, the shared mean)
checked on its own: tests/host_series/series_main.cpp includes nothing but that header, is built with the host compiler — with
the address and undefined-behaviour sanitizers where their runtime links — and run as a child process.  No GPU, no library."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sphexample_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "host_series", "series_main.cpp")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = c and shutil.which(c)
        if path:
            return path
    raise AssertionError("no host C++ compiler found (c++, g++, clang++)")


def test_the_header_is_host_only():
    text = open(os.path.join(CSRC, "sphmi_series.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert '"../../include/sphmi.h"' in includes
    assert not [i for i in includes if "hip" in i or i.startswith('"sphmi_')], includes
    main = [ln.split()[1] for ln in open(MAIN).read().splitlines() if ln.startswith("#include")]
    assert [i for i in main if i.startswith('"')] == ['"sphmi_series.h"']


def test_step_series_under_the_sanitizers(tmp_path):
    cxx = host_compiler()
    exe = str(tmp_path / "series_main")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, MAIN, "-o", exe]
    # the sanitizer runtimes linked statically (a runtime that is a shared library insists on being the first one loaded), then as
    # the compiler links them by default, then — no runtime to link on this machine — none: the assertions still run
    for extra in (SANITIZE + ("-static-libasan", "-static-libubsan"), SANITIZE, ()):
        built = subprocess.run(base + list(extra), capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    print("sanitizers:", " ".join(extra) or "none")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
    assert not run.stderr.strip(), run.stderr               # a sanitizer report would be here
