# TEST INFRASTRUCTURE: the device reader with resident row columns (alignasm_amd/csrc/aasm_read.h under AASM_READ_ROW_COLS) in the
# 1-lane host emulation.  OUT: where the products go.
#   libaasm_emul_read_cols.so  emrc_parse on host arrays, host text or "device" text (read_cols_emul.cpp)
#   read_cols_emul_san         the same in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_read_cols.so: read_cols_emul.cpp $(SRC)/aasm_paf.cpp $(HDRS)
	$(CXX) $(FLAGS) -Wno-unused-result -pthread -Wl,-Bsymbolic read_cols_emul.cpp $(SRC)/aasm_paf.cpp -o $@
$(OUT)/read_cols_emul_san: read_cols_emul.cpp $(SRC)/aasm_paf.cpp $(HDRS)
	$(CXX) $(SAN) -Wno-unused-result -pthread -DAASM_READ_COLS_SAN_MAIN read_cols_emul.cpp $(SRC)/aasm_paf.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_read_cols.so $(OUT)/read_cols_emul_san
.PHONY: clean
