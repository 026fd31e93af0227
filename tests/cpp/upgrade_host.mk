# The upgrade handshake's two host programs (no GPU):
#   upgrade_classes       the C++ classes (WSSession over an in-memory transport)
#                         on a case file, linked against the product library;
#                         tests/test_upgrade_model.py compares the model with it
#   san/test_upgrade_host wsg_upgrade_judge (the rule wsg_upgrade_streams'
#                         kernels run) under AddressSanitizer +
#                         UndefinedBehaviorSanitizer: a program of its own with
#                         the rule's host source instrumented, nothing of
#                         libwsg.so.  Run by tests/test_upgrade_host.py.
#   make -C tests/cpp -f upgrade_host.mk
CXX      ?= g++
ROOT     := ../..
OUT      := _build
CSRC     := $(ROOT)/cppserver_amd/csrc
LIBDIR   := $(abspath $(ROOT)/cppserver_amd/_build)
SAN      := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g -O1

all: $(OUT)/upgrade_classes $(OUT)/san/test_upgrade_host

$(OUT)/upgrade_classes: upgrade_classes.cpp $(wildcard $(ROOT)/include/server/ws/*.h) $(wildcard $(ROOT)/include/server/http/*.h) $(LIBDIR)/libwsg.so
	@mkdir -p $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/include -o $@ upgrade_classes.cpp -L$(LIBDIR) -lwsg -lssl -lcrypto -Wl,-rpath,'$$ORIGIN/../../../cppserver_amd/_build' -pthread

$(OUT)/san/test_upgrade_host: test_upgrade_host.cpp $(CSRC)/wsg_upgrade_host.cpp $(CSRC)/wsg_upgrade.h $(CSRC)/wsg_frame.h $(ROOT)/include/wsg_capi.h
	@mkdir -p $(OUT)/san
	$(CXX) -std=c++17 $(SAN) -Wall -Wextra -I$(ROOT)/include -I$(CSRC) -o $@ test_upgrade_host.cpp $(CSRC)/wsg_upgrade_host.cpp

.PHONY: all
