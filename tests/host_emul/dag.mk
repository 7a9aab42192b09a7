# TEST INFRASTRUCTURE: aasm_topology_sort and aasm_sssp_dag (alignasm_amd/csrc/aasm_sssp.h) in the 1-lane host emulation.
# OUT: where the products go.
#   libaasm_emul_dag.so  graphs_emul.cpp's entries, emk_topology_sort and emk_sssp_dag (dag_emul.cpp)
#   dag_emul_san         the same in a program built with the host address sanitizer, its runtime linked statically
# Flags as in Makefile.
CXX ?= g++
OUT ?= .
SRC := ../../alignasm_amd/csrc
HDRS := emul_launch.h graphs_emul.cpp $(wildcard $(SRC)/*.h $(SRC)/*.hpp) ../../include/alignasm_amd.h
FLAGS := -std=c++17 -O2 -g -Wall -Wno-unused-function -fPIC -shared
SAN := -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan

$(OUT)/libaasm_emul_dag.so: dag_emul.cpp $(HDRS)
	$(CXX) $(FLAGS) dag_emul.cpp -o $@
$(OUT)/dag_emul_san: dag_emul.cpp $(HDRS)
	$(CXX) $(SAN) -DAASM_DAG_SAN_MAIN dag_emul.cpp -o $@
clean:
	rm -f $(OUT)/libaasm_emul_dag.so $(OUT)/dag_emul_san
.PHONY: clean
