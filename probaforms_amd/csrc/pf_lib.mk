# Shared by the Makefiles of the add-on libraries (metrics/csrc, models/*_csrc): each sets LIB and OBJS, says why it is
# compiled with -ffp-contract=off, and includes this.  Builds $(LIB) for gfx950 (MI355X) in-tree; hipcc cross-compiles
# without a GPU.  Every add-on library is kept apart from librnvp_hip.so: its own header and ABI version.
PF_LIB_MK := $(lastword $(MAKEFILE_LIST))
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -ffp-contract=off

all: $(LIB)

# header dependencies come from the compiler (-MMD writes <object>.d next to each object)
%.o: %.hip Makefile $(PF_LIB_MK)
	$(HIPCC) $(CXXFLAGS) -MMD -MP -c $< -o $@

-include $(OBJS:.o=.d)

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

clean:
	rm -f *.o *.d $(LIB)
.PHONY: all clean
