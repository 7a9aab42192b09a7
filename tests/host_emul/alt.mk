# TEST INFRASTRUCTURE: the --alt merge on the device (alignasm_amd/csrc/aasm_alt.h) in the 1-lane host emulation.
# OUT: where the products go.
#   libaasm_emul_alt.so  emalt_merge on the arrays of a host container (alt_emul.cpp)
#   alt_emul_san         the same in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_alt.so: alt_emul.cpp $(SRC)/aasm_paf.cpp $(HDRS)
	$(CXX) $(FLAGS) -Wno-unused-result -pthread -Wl,-Bsymbolic alt_emul.cpp $(SRC)/aasm_paf.cpp -o $@
$(OUT)/alt_emul_san: alt_emul.cpp $(SRC)/aasm_paf.cpp $(HDRS)
	$(CXX) $(SAN) -Wno-unused-result -pthread -DAASM_ALT_SAN_MAIN alt_emul.cpp $(SRC)/aasm_paf.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_alt.so $(OUT)/alt_emul_san
.PHONY: clean
