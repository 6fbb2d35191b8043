# The objects of libkde_hip.so, included by this directory's Makefile and by tools/hooks/Makefile (the stage build of
# the same sources): a new source file is added here and nowhere else.
#   API_OBJS     host code, kde_api*.cpp: the extern "C" surface, one file per family of reference classes
#   KERNEL_OBJS  kernels and their launchers, *.hip
API_OBJS    := kde_api.o kde_api_jbf.o kde_api_dimconv.o kde_api_dasp_ers.o kde_api_pipeline.o kde_api_normals.o kde_api_nasp.o kde_api_les.o kde_api_proj.o kde_api_enh_feed.o kde_api_error3d.o kde_api_cloud.o kde_api_mesh.o kde_api_reg.o kde_api_undist.o kde_api_upsample.o kde_api_holefill.o kde_api_speckle.o kde_api_temporal.o kde_api_decimate.o
KERNEL_OBJS := jbf_kernels.o jbf_fast.o stream_kernels.o dasp_kernels.o ers_kernels.o spdsr_kernels.o normal_kernels.o nasp_kernels.o les_kernels.o proj_kernels.o error3d_kernels.o cloud_kernels.o mesh_kernels.o reg_kernels.o undist_kernels.o upsample_kernels.o holefill_kernels.o speckle_kernels.o temporal_kernels.o decimate_kernels.o
OBJS        := $(API_OBJS) $(KERNEL_OBJS)
