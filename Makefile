# Build: libsimplex.so (gfx950 kernels + C-ABI), the ./solver CLI, and the
# CPU oracle (test infrastructure).  `make -j8`.  Outputs stay in-tree (git-ignored,
# shipped to the GPU box with the snapshot).
# UNITS is the one list of translation units (.hip kernel units and the .cpp host
# runtime, told apart by the source that exists); the compiler writes each
# unit's header dependencies ($(BUILD)/*.d).
ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
ARCH      ?= gfx950
PKG       := simplex_method_gpu_amd
SRC       := $(PKG)/csrc
BUILD     := $(PKG)/_build
HIPFLAGS  := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Iinclude
LDFLAGS   := -L$(ROCM)/lib -Wl,-rpath,$(ROCM)/lib -lrccl

LIB       := $(PKG)/libsimplex.so
# the primal loop's kernel units (make xlib rebuilds these)
KUNITS    := spx_kernels spx_price spx_update spx_foldk
UNITS     := $(KUNITS) spx_reinv spx_tableau spx_loop spx_dual spx_pbox spx_pbox_wexact spx_ranging spx_bndrange spx_api spx_api_dual spx_api_pbox spx_api_ranging
OBJS      := $(UNITS:%=$(BUILD)/%.o)
CLI       := solver
GLPKDRV   := solver_glpk

all: $(LIB) $(CLI) $(GLPKDRV) oracle

$(BUILD)/%.o: $(SRC)/%.hip
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

$(BUILD)/%.o: $(SRC)/%.cpp
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

-include $(OBJS:.o=.d)

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ $(LDFLAGS)

$(CLI): $(SRC)/solver_main.cpp $(SRC)/lp_io.cpp $(SRC)/lp_io.h $(SRC)/mps_io.cpp $(SRC)/mps_io.h include/simplex.h $(LIB)
	g++ -O2 -std=c++17 -Wall -pthread -Iinclude -o $@ $(SRC)/solver_main.cpp $(SRC)/lp_io.cpp $(SRC)/mps_io.cpp -L$(PKG) -Wl,-rpath,'$$ORIGIN/$(PKG)' -lsimplex

# GLPK CPU-baseline counterpart (solver_glpk.cpp): libglpk bound at run time
$(GLPKDRV): $(SRC)/glpk_driver.cpp $(SRC)/lp_io.cpp $(SRC)/lp_io.h
	g++ -O2 -std=c++17 -Wall -pthread -o $@ $(SRC)/glpk_driver.cpp $(SRC)/lp_io.cpp -ldl

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(BUILD) $(LIB) $(CLI) $(GLPKDRV)
	$(MAKE) -C oracle clean

.PHONY: all clean oracle

# Experiment builds (A/B against the default: tools/pass_ab.py, tools/ab_libs.py)
# go to $(AB), which travels to the GPU box only while it exists: `make abclean`
# after the A/B.  (The product ships one libsimplex.so.)
AB        := $(PKG)/_ab

# generic experiment build: make xlib X=name XFLAGS="-DSPX_PRICE_DEEP=0"
# (XFLAGS reach every kernel unit of the primal loop; the rest link as built)
XOBJS     := $(KUNITS:%=$(AB)/x$(X)/%.o)
XREST     := $(filter-out $(KUNITS:%=$(BUILD)/%.o),$(OBJS))
$(AB)/x$(X)/%.o: $(SRC)/%.hip FORCE
	@mkdir -p $(@D)
	$(HIPCC) $(HIPFLAGS) $(XFLAGS) -c $< -o $@
xlib: $(XOBJS) $(XREST)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $(AB)/x$(X)/libsimplex.so $(XOBJS) $(XREST) $(LDFLAGS)

# persistent-loop experiment build: make xloop X=name XFLAGS="-DSPX_LOOP_FU=4"
xloop:
	@mkdir -p $(AB)/l$(X)
	$(HIPCC) $(HIPFLAGS) $(XFLAGS) -c $(SRC)/spx_loop.hip -o $(AB)/l$(X)/spx_loop.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $(AB)/l$(X)/libsimplex.so $(AB)/l$(X)/spx_loop.o $(filter-out %/spx_loop.o,$(OBJS)) $(LDFLAGS)

abclean:
	rm -rf $(AB)

FORCE:
.PHONY: xlib xloop abclean FORCE
