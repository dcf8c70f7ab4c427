"""csrc/small_eig.h on the host: small_eig_host.cpp (a stand-alone program with its own main) includes the header
with its two device qualifiers defined away, is built with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer, and checks jacobi3, svd3_for_umeyama and top_eigvec4 in fp64 on its fixed list.
Nothing is loaded into Python: the program runs as a child process and reports through its exit status."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_small_eig_header_on_the_host_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "small_eig_host")
    # the sanitizer runtimes linked into the program: a dynamic one insists on being the first library loaded
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe,
                            os.path.join(HERE, "small_eig_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "small_eig_host: ok" in run.stdout
