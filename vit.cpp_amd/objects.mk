# The objects of libvitx.so, by source name under csrc/ -- the one list both vit.cpp_amd/Makefile and tools/Makefile build from.
VITX_OBJS = gemm gemm_ring gemm_pp gemm_mx8 layernorm attention attention_single attention_flow attention_persist attention_generic attention_cls \
            attention_packed attention_stream attention_map attention_pool attention_text text_embed features zeroshot nn_select dense_label depth_map pos_resample rope swiglu patch_embed quant softmax_topk image_preprocess probe \
            tuning weights context forward heads text_forward packed_context packed_forward packed_outputs packed_input outputs ops depth_host model_file quantize mxfp8 pos_resample_host preprocess vit_api sharded image_decode
