# The objects of libvitx.so, by source name under csrc/ -- the one list both vit.cpp_amd/Makefile and tools/Makefile build from.
VITX_OBJS = kernels attention_stream attention_map features pos_resample gemm_ring gemm_pp gemm_mx8 patch_embed quant probe \
            context forward outputs ops model_file quantize mxfp8 pos_resample_host preprocess vit_api sharded image_decode
