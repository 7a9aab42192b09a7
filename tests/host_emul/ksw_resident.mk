# TEST INFRASTRUCTURE: k shortest walks on a resident graph batch (alignasm_amd/csrc/aasm_graphs.h: graphs_ksw / graphs_ksw_export) in
# the host emulation.  OUT: where the products go.
#   libaasm_emul_ksw_resident.so  graphs_resident_emul.cpp's entries with the k-walk solve and export (ksw_resident_emul.cpp)
#   ksw_resident_emul_san         the same in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h graphs_emul.cpp graphs_resident_emul.cpp $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_ksw_resident.so: ksw_resident_emul.cpp $(HDRS)
	$(CXX) $(FLAGS) ksw_resident_emul.cpp -o $@
$(OUT)/ksw_resident_emul_san: ksw_resident_emul.cpp $(HDRS)
	$(CXX) $(SAN) -DAASM_KSWR_SAN_MAIN ksw_resident_emul.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_ksw_resident.so $(OUT)/ksw_resident_emul_san
.PHONY: clean
