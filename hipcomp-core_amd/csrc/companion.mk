# The build of one companion library of libhipcomp.so, hipcomp-core_amd/lib/libhipcomp_$(NAME).so for gfx950
# (cross-compiles without a GPU), with the same flags as ./Makefile.  csrc/$(NAME)/Makefile sets what is its own
# and includes this file:
#   NAME     the directory under csrc/ and the library's suffix; the sources are $(NAME)_kernels.hip and
#            $(NAME)_batch.cpp, the exports $(NAME)/exports.map
#   INCDIRS  further include directories, after the directory's own
#   DEPLIBS, LDLIBS  (gzip only) libraries it links: the files to wait for, and the link flags
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT     := $(abspath $(CSRC)/../..)
SRCDIR   := $(CSRC)/$(NAME)
OUTDIR   := $(ROOT)/hipcomp-core_amd/lib
OBJDIR   := $(SRCDIR)/build
CXXFLAGS := -std=c++17 -O3 -fPIC -I$(ROOT)/include -I$(CSRC) -I$(SRCDIR) $(addprefix -I,$(INCDIRS)) \
            -Wall -Wno-unused-function -fno-strict-aliasing $(EXTRA)

OBJS     := $(OBJDIR)/$(NAME)_kernels.hip.o $(OBJDIR)/$(NAME)_batch.cpp.o

all: $(OUTDIR)/libhipcomp_$(NAME).so

# As in ./Makefile: the device assembly of the very object that ships is kept and has to pass the hazard
# check before the object is accepted.  The headers an object depends on are those the compiler read for it,
# written next to it as a .d file (named for the final object, not the one in _temps) and included below.
$(OBJDIR)/%.hip.o: $(SRCDIR)/%.hip $(CSRC)/check_asm_hazards.py
	@mkdir -p $(OBJDIR)/$*_temps
	$(HIPCC) $(CXXFLAGS) --offload-arch=$(ARCH) -save-temps=obj -MMD -MP -MT $@ -MF $(OBJDIR)/$*.hip.d \
	    -c $< -o $(OBJDIR)/$*_temps/$*.hip.o
	python3 $(CSRC)/check_asm_hazards.py $(OBJDIR)/$*_temps/$*-hip-amdgcn-amd-amdhsa-$(ARCH).s
	cp $(OBJDIR)/$*_temps/$*-hip-amdgcn-amd-amdhsa-$(ARCH).s $(OBJDIR)/$*.$(ARCH).s
	mv $(OBJDIR)/$*_temps/$*.hip.o $@
	rm -rf $(OBJDIR)/$*_temps

$(OBJDIR)/%.cpp.o: $(SRCDIR)/%.cpp
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) -x hip --offload-arch=$(ARCH) -MMD -MP -MT $@ -MF $(OBJDIR)/$*.cpp.d -c $< -o $@

$(OUTDIR)/libhipcomp_$(NAME).so: $(OBJS) $(SRCDIR)/exports.map $(DEPLIBS)
	@mkdir -p $(OUTDIR)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -Wl,--version-script=$(SRCDIR)/exports.map $(OBJS) $(LDLIBS) -o $@

clean:
	rm -rf $(OBJDIR) $(OUTDIR)/libhipcomp_$(NAME).so

.PHONY: all clean

-include $(OBJS:.o=.d)
