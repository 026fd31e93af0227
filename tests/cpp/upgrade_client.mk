# The client upgrade's host programs (no GPU):
#   upgrade_client_classes       the C++ classes (WSClient over an in-memory
#                                transport) on a case file, linked against the
#                                product library; tests/test_upgrade_client_model.py
#                                compares the model with it
#   san/test_upgrade_client_host wsg_upgrade_client_judge and wsg_upgrade_request
#                                (the rule the kernels run) under AddressSanitizer
#                                + UndefinedBehaviorSanitizer: a program of its own
#                                with the rule's host source instrumented, nothing
#                                of libwsg.so
#   san/test_upgrade_client_args args_upgrade_client / args_upgrade_requests
#                                with a recording in_alloc, the same way
# The last two are run by tests/test_upgrade_client_host.py.
#   make -C tests/cpp -f upgrade_client.mk
CXX      ?= g++
ROOT     := ../..
OUT      := _build
CSRC     := $(ROOT)/cppserver_amd/csrc
LIBDIR   := $(abspath $(ROOT)/cppserver_amd/_build)
SAN      := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g -O1

all: $(OUT)/upgrade_client_classes $(OUT)/san/test_upgrade_client_host $(OUT)/san/test_upgrade_client_args

$(OUT)/upgrade_client_classes: upgrade_client_classes.cpp $(wildcard $(ROOT)/include/server/ws/*.h) $(wildcard $(ROOT)/include/server/http/*.h) $(LIBDIR)/libwsg.so
	@mkdir -p $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/include -o $@ upgrade_client_classes.cpp -L$(LIBDIR) -lwsg -lssl -lcrypto -Wl,-rpath,'$$ORIGIN/../../../cppserver_amd/_build' -pthread

$(OUT)/san/test_upgrade_client_host: test_upgrade_client_host.cpp $(CSRC)/wsg_upgrade_client_host.cpp $(CSRC)/wsg_upgrade_client.h $(CSRC)/wsg_upgrade.h $(CSRC)/wsg_frame.h $(ROOT)/include/wsg_capi.h
	@mkdir -p $(OUT)/san
	$(CXX) -std=c++17 $(SAN) -Wall -Wextra -I$(ROOT)/include -I$(CSRC) -o $@ test_upgrade_client_host.cpp $(CSRC)/wsg_upgrade_client_host.cpp

$(OUT)/san/test_upgrade_client_args: test_upgrade_client_args.cpp $(CSRC)/wsg_args.h $(CSRC)/wsg_operands.h $(ROOT)/include/wsg_capi.h
	@mkdir -p $(OUT)/san
	$(CXX) -std=c++17 $(SAN) -Wall -Wextra -I$(ROOT)/include -I$(CSRC) -o $@ test_upgrade_client_args.cpp

.PHONY: all
