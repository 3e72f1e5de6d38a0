"""The pure host rules of the image front end (putslam_amd/csrc/ps_image_rule.h: PsImageSet strides, row stride and addressable
bytes of a host image, the limits, the block layout) compiled into a plain C++ program -- no HIP header, no GPU -- and run:
tests/cpp/test_image_rule.cpp holds the cases."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_rule_program(tmp_path):
    exe = str(tmp_path / "test_image_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_image_rule.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "image rule ok", run.stdout
