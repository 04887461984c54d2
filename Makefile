# Build libislpose.so (HIP, gfx950) in-tree, and the oracle's reference build helpers.
HIPCC    ?= /opt/rocm/bin/hipcc
HOSTCXX  ?= /opt/rocm/llvm/bin/clang++
ARCH     ?= gfx950
PKG      := isl-signlanguage-translation_amd
CSRC     := $(PKG)/csrc
OUT      := $(PKG)/islpose/libislpose.so
# -ffp-contract=off: the post-processing kernels reproduce numpy/OpenCV fp32/fp64
# operation order bit-for-bit, which forbids fused multiply-adds.
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -Iinclude -I$(CSRC) \
            -Wall -Wno-unused-function -Wno-unused-variable -Wno-unused-lambda-capture
SRCS     := $(CSRC)/conv.hip $(CSRC)/conv_x3.hip $(CSRC)/conv_c12.hip $(CSRC)/wino_f16.hip $(CSRC)/wino.hip $(CSRC)/ops.hip $(CSRC)/post.hip $(CSRC)/sign.hip $(CSRC)/sign_train.hip $(CSRC)/sign_augment.hip $(CSRC)/augment.hip $(CSRC)/draw.hip $(CSRC)/pack.cpp $(CSRC)/x3_select.cpp $(CSRC)/post_plan.cpp $(CSRC)/runtime.cpp
OBJS     := $(patsubst $(CSRC)/%,build/%.o,$(SRCS))
# development objects (tools/convbench): the product sources plus the rejected split-fp16
# Winograd kernel and the s_memtime stamp variant, compiled with -DISLPOSE_DEV
DEV_SRCS := $(SRCS) $(CSRC)/wino_x3.hip
DEV_OBJS := $(patsubst $(CSRC)/%,build_dev/%.o,$(DEV_SRCS))

all: $(OUT)

HDRS     := $(CSRC)/internal.h $(CSRC)/x3_select.h $(CSRC)/pack.h $(CSRC)/sign_common.h include/islpose.h

# (post_plan.h: the sizing constants, switches, plans and scratch layouts of the post)
build/post.hip.o build/post_plan.cpp.o build_dev/post.hip.o build_dev/post_plan.cpp.o: $(CSRC)/post_plan.h

# (x3_instances.h: the instance table of the split-fp16 kernels and its host-side copy)
build/conv_x3.hip.o build/x3_select.cpp.o build_dev/conv_x3.hip.o build_dev/x3_select.cpp.o: $(CSRC)/x3_instances.h

build/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OUT): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -Wl,-z,defs -o $@ $(OBJS)

build_dev/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p build_dev
	$(HIPCC) $(HIPFLAGS) -DISLPOSE_DEV -x hip -c $< -o $@

# development library (ISLPOSE_LIB=tools/libislpose_dev.so: tools/tile_prof.py)
tools/libislpose_dev.so: $(DEV_OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -Wl,-z,defs -o $@ $^

clean:
	rm -rf build build_dev $(OUT)

.PHONY: all clean

# development microbenchmark of the conv kernels (not part of the library)
tools/convbench: tools/convbench.cpp $(DEV_OBJS)
	$(HIPCC) $(HIPFLAGS) -DISLPOSE_DEV -x hip tools/convbench.cpp -x none $(DEV_OBJS) -o $@

# digests of the weight packs on the CPU (tests/test_pack.py): host compiler only, no device
tools/pack_digest: tools/pack_digest.cpp $(CSRC)/pack.cpp $(CSRC)/pack.h
	$(HOSTCXX) -O2 -std=c++17 -ffp-contract=off -Wall -I$(CSRC) tools/pack_digest.cpp $(CSRC)/pack.cpp -o $@

# what launch_conv_x3 would run for a launch, and the sweep that holds the instance table closed
# under the decision (tests/test_x3_select.py): host compiler only, no device
tools/x3_choice: tools/x3_choice.cpp $(CSRC)/x3_select.cpp $(CSRC)/x3_select.h $(CSRC)/x3_instances.h
	$(HOSTCXX) -O2 -std=c++17 -ffp-contract=off -Wall -I$(CSRC) tools/x3_choice.cpp $(CSRC)/x3_select.cpp -o $@

# the plans and scratch layouts of the post-processing for a geometry (tests/test_post_plan.py):
# host compiler only, no device
tools/post_plan: tools/post_plan.cpp $(CSRC)/post_plan.cpp $(CSRC)/post_plan.h include/islpose.h
	$(HOSTCXX) -O2 -std=c++17 -ffp-contract=off -Wall -Iinclude -I$(CSRC) tools/post_plan.cpp $(CSRC)/post_plan.cpp -o $@
