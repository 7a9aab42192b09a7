# TEST INFRASTRUCTURE: aasm_sssp_bellman_ford and k shortest walks with AASM_KSW_NEGATIVE (alignasm_amd/csrc/aasm_sssp.h, aasm_ksw.h)
# in the 1-lane host emulation.  OUT: where the products go.
#   libaasm_emul_bf.so  graphs_emul.cpp's entries and emk_sssp_bellman_ford (bf_emul.cpp)
#   bf_emul_san         the same in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h graphs_emul.cpp $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_bf.so: bf_emul.cpp $(HDRS)
	$(CXX) $(FLAGS) bf_emul.cpp -o $@
$(OUT)/bf_emul_san: bf_emul.cpp $(HDRS)
	$(CXX) $(SAN) -DAASM_BF_SAN_MAIN bf_emul.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_bf.so $(OUT)/bf_emul_san
.PHONY: clean
