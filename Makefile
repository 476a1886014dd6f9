# Build of the MI355X ISSL scorer: libissl_hip.so (C ABI, include/issl_hip.h; libissl_hip.map keeps every other symbol
# out of its dynamic table), the three drop-in executables, isslReportOfftargets, isslLocateOfftargets, isslLandOfftargets,
# isslSearchGenome, isslIndexFromFasta,
# cracklingGuides, cracklingBowtie and countHitTranscripts.  hipcc cross-compiles for gfx950 without a GPU present.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC     = crackling_amd/csrc
# -ffp-contract=off: the reference is built without FMA (Makefile:5, x86-64 baseline); the
# MIT/CFD doubles must round the same way on host and device.
CXXFLAGS = -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result
HIPFLAGS = $(CXXFLAGS) --offload-arch=$(ARCH)
LIB      = crackling_amd/libissl_hip.so

all: $(LIB) bin/isslScoreOfftargets bin/isslReportOfftargets bin/isslLocateOfftargets bin/isslLandOfftargets bin/isslSearchGenome bin/isslCreateIndex bin/extractOfftargets bin/isslIndexFromFasta bin/cracklingGuides bin/cracklingBowtie bin/countHitTranscripts

# The library: one object per source under build/obj/, the same flags for kernels and host code; the header dependencies
# come from the compiler (-MMD -MP).
SRCS = issl_kernels.hip issl_bin.hip issl_verify.hip issl_group.hip issl_replay.hip issl_report.hip issl_extract.hip \
       issl_locate.hip issl_search.hip issl_bulge.hip issl_variants.hip issl_bulge_variants.hip issl_haplotypes.hip issl_landing.hip issl_occur.hip issl_guides.hip issl_consensus.hip issl_build.hip issl_transcripts.hip issl_results.hip issl_results.cpp issl_folds.hip issl_folds.cpp issl_runlog.hip issl_annotation.cpp issl_capi.cpp issl_upload.cpp issl_pipeline.cpp issl_options.cpp issl_host.cpp issl_text.cpp issl_node.cpp
OBJDIR = build/obj
OBJS   = $(addprefix $(OBJDIR)/,$(addsuffix .o,$(SRCS)))  # (the suffix stays in the name: issl_results.hip and issl_results.cpp)
COMPILE = $(HIPCC) $(HIPFLAGS) -MMD -MP -c -o $@ $<

$(OBJDIR):
	mkdir -p $@
$(OBJDIR)/%.hip.o: $(CSRC)/%.hip | $(OBJDIR)
	$(COMPILE)
$(OBJDIR)/%.cpp.o: $(CSRC)/%.cpp | $(OBJDIR)
	$(COMPILE)

$(LIB): $(OBJS) $(CSRC)/libissl_hip.map
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJS) -Wl,--version-script=$(CSRC)/libissl_hip.map -lpthread -ldl

-include $(OBJS:.o=.d)

# The host-only executables: libissl_hip.so is loaded with dlopen (cli_api.hpp: the search for the library, the symbols each
# one needs, the ABI check) -- by isslScoreOfftargets only when the process has to score by itself, not when a resident
# server answers (cli_score.cpp).  One recipe for the eight, each behind its own source:
#   isslScoreOfftargets   the drop-in scorer                 isslReportOfftargets  the off-target report (records or --profile)
#   isslLocateOfftargets  where the off-targets lie          cracklingGuides       the candidate guides of FASTA inputs
#   cracklingBowtie       the Bowtie step for a guide list   countHitTranscripts   transcript hit counts for Crackling's output
#   isslLandOfftargets    off-target landings: guide, site, place in the genome, transcript hits (records or --profile)
#   isslSearchGenome      index-free search: any PAM pattern, any length up to 32, up to k mismatches, with --guide also DNA and
#                         RNA bulges, with --variants / --vcf IUPAC codes in the text and SNPs of a VCF, with --guide-variants /
#                         --guide-vcf both together, with --indel-vcf the ALT haplotypes of a VCF's indels (rows or --profile)
DLOPEN_EXES = bin/isslScoreOfftargets bin/isslReportOfftargets bin/isslLocateOfftargets bin/cracklingGuides bin/cracklingBowtie \
              bin/countHitTranscripts bin/isslLandOfftargets bin/isslSearchGenome
bin/isslScoreOfftargets: $(CSRC)/cli_score.cpp $(CSRC)/issl_host.hpp
bin/isslReportOfftargets: $(CSRC)/cli_report.cpp
bin/isslLocateOfftargets: $(CSRC)/cli_locate.cpp
bin/cracklingGuides: $(CSRC)/cli_guides.cpp
bin/cracklingBowtie: $(CSRC)/cli_bowtie.cpp
bin/countHitTranscripts: $(CSRC)/cli_transcripts.cpp
bin/isslLandOfftargets: $(CSRC)/cli_landing.cpp
bin/isslSearchGenome: $(CSRC)/cli_search.cpp $(CSRC)/issl_search_text.hpp $(CSRC)/issl_variants_text.hpp $(CSRC)/issl_bulge_variants_text.hpp $(CSRC)/issl_haplotypes_text.hpp
$(DLOPEN_EXES): $(CSRC)/cli_api.hpp include/issl_hip.h $(LIB)
	@mkdir -p bin
	g++ $(CXXFLAGS) -o $@ $(filter %.cpp,$^) -lpthread -ldl

bin/extractOfftargets: $(CSRC)/cli_extract.cpp $(CSRC)/cli_inputs.hpp $(LIB)
	@mkdir -p bin
	$(HIPCC) $(CXXFLAGS) -o $@ $< -Lcrackling_amd -lissl_hip -Wl,-rpath,'$$ORIGIN/../crackling_amd'

bin/isslIndexFromFasta: $(CSRC)/cli_index_fasta.cpp $(CSRC)/cli_inputs.hpp include/issl_hip.h $(LIB)
	@mkdir -p bin
	$(HIPCC) $(CXXFLAGS) -o $@ $< -Lcrackling_amd -lissl_hip -Wl,-rpath,'$$ORIGIN/../crackling_amd'

# host-only executable: no HIP runtime behind it (start-up of libamdhip64 alone costs ~1.5 s)
bin/isslCreateIndex: $(CSRC)/cli_create.cpp $(CSRC)/issl_host.cpp $(CSRC)/issl_host.hpp
	@mkdir -p bin
	g++ $(CXXFLAGS) -o $@ $(CSRC)/cli_create.cpp $(CSRC)/issl_host.cpp -lpthread

oracle:
	$(MAKE) -C oracle all

clean:
	rm -rf $(LIB) bin $(OBJDIR)
.PHONY: all oracle clean
