# Builds the packed-scan mirror test (run by tests/test_pack_mirror.py).
CXX ?= g++
ROOT = ../..
pack_mirror_test: pack_mirror_test.cpp $(ROOT)/go-lsm_amd/libgolsm.so
	$(CXX) -O2 -std=c++17 -Wall -I$(ROOT)/include -I$(ROOT)/go-lsm_amd/host \
	    -o $@ pack_mirror_test.cpp -L$(ROOT)/go-lsm_amd -lgolsm -llsm_gpu \
	    -Wl,-rpath,'$$ORIGIN/$(ROOT)/go-lsm_amd' -lpthread
