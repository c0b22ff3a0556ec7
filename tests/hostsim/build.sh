#!/bin/bash
# builds the TEST-ONLY host twin of the solver core (see hostsim.cpp header)
set -e
cd "$(dirname "$0")"
if [ ! -f libhostsim.so ] || [ hostsim.cpp -nt libhostsim.so ] || [ hostsim_scaled.cpp -nt libhostsim.so ] || [ ../../myriad_amd/csrc/hs_solver.h -nt libhostsim.so ] || [ ../../myriad_amd/csrc/ip_policy.h -nt libhostsim.so ] || [ ../../myriad_amd/csrc/bound_rules.h -nt libhostsim.so ] || [ ../../myriad_amd/csrc/systems_gen.h -nt libhostsim.so ] || [ ../../myriad_amd/csrc/rollout.h -nt libhostsim.so ] || [ ../../myriad_amd/csrc/os_solver.h -nt libhostsim.so ]; then
  # two translation units, compiled side by side (hostsim_scaled.cpp: the lane cores of 14 systems under a variable scale)
  g++ -O2 -std=c++17 -fopenmp -fPIC -c hostsim.cpp -o hostsim.o &
  g++ -O2 -std=c++17 -fopenmp -fPIC -c hostsim_scaled.cpp -o hostsim_scaled.o
  wait $!
  g++ -fopenmp -shared hostsim.o hostsim_scaled.o -o libhostsim.so
fi
