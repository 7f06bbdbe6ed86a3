# Builds the database-scan mirror test (run by tests/test_db_scan_mirror.py).
CXX ?= g++
ROOT = ../..
db_scan_mirror_test: db_scan_mirror_test.cpp $(ROOT)/go-lsm_amd/libgolsm.so
	$(CXX) -O2 -std=c++17 -Wall -I$(ROOT)/include -I$(ROOT)/go-lsm_amd/host \
	    -o $@ db_scan_mirror_test.cpp -L$(ROOT)/go-lsm_amd -lgolsm -llsm_gpu \
	    -Wl,-rpath,'$$ORIGIN/$(ROOT)/go-lsm_amd' -lpthread
