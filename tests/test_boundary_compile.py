"""SURVEY.md §8(b), first sentence: the reference application must compile UNCHANGED against this build's
Controller / ProgramHandler / Logger / FileHandler / Comparator headers and CL/cl.h.

The application is compiled where it lies by oracle/Makefile (target `ref`, run by build() where the reference tree
exists; its source is never copied), against host/include plus a test-only declaration stub of the few cv:: names it
uses (tests/stubs/opencv2: OpenCV is not installed here), into oracle/_ref/RealtimeImageProcessing.o, which travels
with oracle/_ref.  This is an interface check, not a parity check: the first test is skipped where oracle/_ref was not
built; the second needs nothing but g++."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as entry

HOST_INC = os.path.join(entry.PKG_DIR, "host", "include")
HOST_LIB = os.path.join(entry.PKG_DIR, "lib", "libmi355_host.so")
STUBS = os.path.join(entry.ROOT, "tests", "stubs")
APP_OBJ = os.path.join(entry.ROOT, "oracle", "_ref", "RealtimeImageProcessing.o")
APP_ERR = os.path.join(entry.ROOT, "oracle", "_ref", "RealtimeImageProcessing.err")
HOST_CLASSES = ("Controller::", "ProgramHandler::", "Logger::", "FileHandler::", "Comparator::")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not present on this machine")


def _nm(*args):
    """Mangled symbol names nm lists (no spaces in them: the name is the line's last field)."""
    run = subprocess.run(["nm"] + list(args), capture_output=True, text=True, check=True)
    return [ln.split()[-1] for ln in run.stdout.splitlines() if ln.strip()]


def _demangle(symbols):
    run = subprocess.run(["c++filt"], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True)
    return run.stdout.splitlines()


def test_reference_application_compiles_unchanged_against_the_host_headers():
    """The object oracle/Makefile compiled, and every host-API symbol it leaves undefined (the Controller /
    ProgramHandler / Logger / FileHandler / Comparator members and the cl* calls; cv:: and the C++ runtime aside)
    is exported by lib/libmi355_host.so."""
    if not os.path.exists(APP_OBJ):
        if os.path.exists(APP_ERR):
            pytest.fail("the reference application does not compile against host/include:\n" + open(APP_ERR).read()[-4000:])
        pytest.skip("oracle/_ref not built here")
    undefined = _nm("-u", APP_OBJ)
    names = dict(zip(undefined, _demangle(undefined)))
    wanted = sorted(m for m, d in names.items() if d.startswith(HOST_CLASSES) or d.startswith("cl"))
    assert wanted, names
    exported = set(_nm("-D", "--defined-only", HOST_LIB))
    assert [names[m] for m in wanted if m not in exported] == []


@needs_gxx
def test_every_member_the_application_calls_is_declared_with_the_reference_signature(tmp_path):
    """Belt and braces for the check above: take the address of every Controller / ProgramHandler / Logger member
    RealtimeImageProcessing.cpp:435-442,351-355,372-376,398-402,423-426 uses, with the exact pointer-to-member
    types of the reference headers (include/Controller.hpp:37-47, include/ProgramHandler.hpp:9-22)."""
    src = tmp_path / "sig.cpp"
    src.write_text(r'''
#include <ProgramHandler.hpp>
#include <FileHandler.hpp>
#include <Comparator.hpp>
using V8 = std::vector<unsigned char>;
using VU = std::vector<cl_ulong>;
void (Controller::*g)(cl_context*, cl_command_queue*, cl_kernel*, VU*, V8*, V8*, cl_int&, cl_int&, Logger&) =
    &Controller::PerformCLImageGrayscaling;
void (Controller::*e)(cl_context*, cl_command_queue*, cl_kernel*, VU*, V8*, V8*, cl_int&, cl_int&, Logger&) =
    &Controller::PerformCLImageEdgeDetection;
void (Controller::*b)(int&, float&, cl_context*, cl_command_queue*, cl_kernel*, VU*, V8*, V8*, cl_int&, cl_int&,
                      Logger&) = &Controller::PerformCLGaussianBlur;
cl_bool (Controller::*gi)() = &Controller::GetImageSupport;
void (ProgramHandler::*io)(Controller&, cl_context*, cl_command_queue*, cl_program*, cl_kernel*, std::string,
                           Logger&) = &ProgramHandler::InitOpenCL;
V8 (ProgramHandler::*po)(Controller&, const cv::Mat&, cl_context*, cl_command_queue*, cl_kernel*, cl_int&, cl_int&,
                         Logger&, std::string) = &ProgramHandler::PerformOpenCL;
V8 (ProgramHandler::*pi)(Controller&, std::string, cl_context*, cl_command_queue*, cl_kernel*, double&, double&,
                         double&, double&, double&, cl_int&, cl_int&, Logger&, std::string) =
    &ProgramHandler::PerformOpenCL;
void (ProgramHandler::*ak)(std::vector<std::string>, std::string) = &ProgramHandler::AddKernels;
void (ProgramHandler::*sd)(int, int) = &ProgramHandler::SetDeviceProperties;
void (ProgramHandler::*il)(Logger&, Logger::LogLevel, bool) = &ProgramHandler::InitLogger;
cv::Mat (Comparator::*cg)(std::string, double&, Logger&) = &Comparator::PerformCPU_Grayscaling;
std::vector<std::string> (FileHandler::*li)(const std::string&) = &FileHandler::LoadImages;
cl_int (*r1)(cl_kernel) = &clReleaseKernel;
cl_int (*r2)(cl_program) = &clReleaseProgram;
cl_int (*r3)(cl_command_queue) = &clReleaseCommandQueue;
cl_int (*r4)(cl_context) = &clReleaseContext;
int main() { ProgramHandler ph(1, false, false, true, true); (void)ph; return 0; }
''')
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-I", HOST_INC, "-I", STUBS, str(src)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
