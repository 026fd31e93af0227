# wsg_proto_judge (the rule wsg_check_protocol's kernels run) under
# AddressSanitizer + UndefinedBehaviorSanitizer: a program of its own with the
# rule's host source instrumented; no GPU, nothing of libwsg.so.  Run by
# tests/test_protocol_host.py.
#   make -C tests/cpp -f proto_host.mk
CXX      ?= g++
ROOT     := ../..
OUT      := _build
CSRC     := $(ROOT)/cppserver_amd/csrc
SAN      := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g -O1

all: $(OUT)/san/test_proto_host

$(OUT)/san/test_proto_host: test_proto_host.cpp $(CSRC)/wsg_proto_host.cpp $(CSRC)/wsg_proto.h $(CSRC)/wsg_frame.h $(ROOT)/include/wsg_capi.h
	@mkdir -p $(OUT)/san
	$(CXX) -std=c++17 $(SAN) -Wall -Wextra -I$(ROOT)/include -I$(CSRC) -o $@ test_proto_host.cpp $(CSRC)/wsg_proto_host.cpp

.PHONY: all
