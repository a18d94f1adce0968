#!/bin/bash
# Builds the host units (csrc/tgnh_*.cpp), the launch stubs and the stand-alone driver host_driver.cpp into ONE program with
# AddressSanitizer + UBSan (g++, CPU only) and runs it: the host side of tgnh_set_temperatures / tgnh_set_velocities_to_temperature,
# the molecule table, the periodic box and the frame's argument checks.
set -e
cd "$(dirname "$0")/../.."
OUT=$(mktemp -d)/tgnh_host_driver
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ \
    -I/opt/rocm/include openmm_drudenose_amd/csrc/tgnh_*.cpp tools/sanitize/launch_stubs.cpp tools/sanitize/host_driver.cpp \
    -L/opt/rocm/lib -lamdhip64 -ldl -Wl,-rpath,/opt/rocm/lib -o "$OUT"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT"
