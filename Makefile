# Builds the gfx950 kernel library (product) and nothing else.  hipcc cross-compiles without a GPU.
HIPCC ?= hipcc
ARCH  ?= gfx950
CSRC  := dahitra_amd/csrc
OBJ   := build/obj
LIB   := dahitra_amd/lib/libdahitra_hip.so
SRCS  := $(wildcard $(CSRC)/*.hip)
OBJS  := $(patsubst $(CSRC)/%.hip,$(OBJ)/%.o,$(SRCS))
FLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -Wno-unused-result

all: $(LIB)

# the token-side kernels are long dependent chains at one or two waves per SIMD: schedule them for ILP, not occupancy
# (fused encoder forward 66.9 -> 50.7 us)
ILP_SRCS := encoder_fused tokens
$(foreach f,$(ILP_SRCS),$(eval $(OBJ)/$(f).o: EXTRA := -mllvm -amdgpu-sched-strategy=max-ilp))

# fused decoder: MFMA results in VGPRs (its small products feed VALU chains at once: the AGPR form costs a v_accvgpr_read per
# value, 8 % of the forward's instructions, and two waves per SIMD of occupancy at MLP 64); since the two-workgroups-per-CU
# rewrite the default scheduler beats max-ilp on the backward (no scratch at 248 registers: 38.5 -> 37.3 / 8.8 -> 7.9 us)
$(OBJ)/decoder_fused.o: EXTRA := -mllvm -amdgpu-mfma-vgpr-form

# norm: its one MFMA kernel (head_bn_bwd_kernel) hands every result to the vector ALU at once
$(OBJ)/norm.o: EXTRA := -mllvm -amdgpu-mfma-vgpr-form

# conv_wreg: its stream loop is ONE fully unrolled tile (up to 1152 steps); the default pragma-unroll budget (16 K instructions)
# silently falls back to a partial unroll, which turns the register-resident weight array into scratch memory
# ... and no SLP packing of fp32 chains into v_pk_*_f32: conv3x3_up4_wreg32_kernel returned wrong bits from run to run with it (see the
# note at that kernel); the other kernels of the file are bit-identical and time-neutral under the flag
$(OBJ)/conv_wreg.o: EXTRA := -mllvm -pragma-unroll-threshold=262144 -fno-slp-vectorize

# augment_xbd_colour: its float64 blends and float32 HSV return are byte contracts stated product by product; a fused multiply-add
# (hipcc contracts by default) rounds once where they round twice
$(OBJ)/augment_xbd_colour.o: EXTRA := -ffp-contract=off

$(OBJ)/%.o: $(CSRC)/%.hip $(CSRC)/common.h $(CSRC)/conv_mfma_impl.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(FLAGS) $(EXTRA) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

clean:
	rm -rf build $(LIB)

.PHONY: all clean
