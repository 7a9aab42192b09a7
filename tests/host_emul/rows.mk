# TEST INFRASTRUCTURE: the rows kernels (alignasm_amd/csrc/aasm_rows.h) in the 1-lane host emulation.  OUT: where the products go.
#   libaasm_emul_rows.so  emw_rows_sizes / emw_rows_format on host arrays (rows_emul.cpp)
#   rows_emul_san         the same bodies in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_rows.so: rows_emul.cpp $(HDRS)
	$(CXX) $(FLAGS) rows_emul.cpp -o $@
$(OUT)/rows_emul_san: rows_emul.cpp $(HDRS)
	$(CXX) $(SAN) -DAASM_ROWS_SAN_MAIN rows_emul.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_rows.so $(OUT)/rows_emul_san
.PHONY: clean
