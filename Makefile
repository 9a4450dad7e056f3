# Build libhdpgpc_hip.so (gfx950).  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC   = hdpgpc_amd/csrc
SRCS   = $(wildcard $(CSRC)/*.hip)
HDR    = $(CSRC)/tile_f64.hpp $(CSRC)/hgp_internal.hpp $(CSRC)/panel_prod.hpp $(CSRC)/hgp_segops.hpp $(wildcard include/*.h)
OBJDIR = build/obj
OBJS   = $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
LIB    = hdpgpc_amd/lib/libhdpgpc_hip.so
FLAGS  = -O3 --offload-arch=$(ARCH) -mllvm -pragma-unroll-threshold=1048576 -fPIC -Wno-unused-result

all: $(LIB)

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDR)
	mkdir -p $(OBJDIR)
	$(HIPCC) $(FLAGS) -c -o $@ $<

# the ragged pair kernels are the templates of the rectangular units, instantiated in units of their own
$(OBJDIR)/hgp_pairs_ragged.o: $(CSRC)/hgp_pairs.hip
$(OBJDIR)/hgp_pairs_acc_ragged.o: $(CSRC)/hgp_pairs_acc.hip
# and so is the streamed band kernel of the segment-operator store
$(OBJDIR)/hgp_segops.o: $(CSRC)/hgp_pairs.hip

$(LIB): $(OBJS)
	mkdir -p hdpgpc_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

# diagnostic build with in-kernel cycle stamps (tools/stamps.py); never used by the product path
stamps: $(SRCS) $(HDR)
	mkdir -p hdpgpc_amd/lib/ab
	$(HIPCC) $(FLAGS) -DHGP_STAMPS -shared -o hdpgpc_amd/lib/ab/libhgp_stamps.so $(SRCS)

# every workgroup barrier followed by a pseudo-random per-wave delay: run the GPU tests with HGP_LIB pointing at it
racestress: $(SRCS) $(HDR)
	mkdir -p hdpgpc_amd/lib/ab
	$(HIPCC) $(FLAGS) -DHGP_RACE_STRESS -shared -o hdpgpc_amd/lib/ab/libhgp_race_stress.so $(SRCS)

clean:
	rm -rf $(LIB) $(OBJDIR)
