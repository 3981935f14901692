# oracle/_ref/adapter_test: integration/redset_hip_backend.c (the
# reference-signature backend slot) linked into a test driver
# (tests/adapter/adapter_test.c) that calls it with redset's own types. It
# needs the reference's headers, so __graft_entry__.build() runs this recipe
# only where they exist; oracle/_ref/ is kept out of git, and the built binary
# travels with the tree to where the GPU tests run. Nothing of the reference
# is compiled: only our two .c files, against its declarations.
# usage: make -C oracle -f adapter_test.mk REF_SRC=<the reference's src/>
ifeq ($(REF_SRC),)
$(error REF_SRC must name the reference's src/ directory)
endif
MPI_HOME ?= /opt/conda
LIBDIR   := ../redset_amd/lib
INC      := -I../tests/integration_stubs -I$(REF_SRC) -I../include -I../integration -I$(MPI_HOME)/include
all: _ref/adapter_test
_ref/adapter_test: ../tests/adapter/adapter_test.c ../integration/redset_hip_backend.c ../integration/redset_hip_backend.h \
                   ../include/redset_hip.h ../include/redset_hip_mpi.h $(LIBDIR)/libredset_hip_mpi.so
	@mkdir -p _ref
	gcc -O2 -std=gnu99 -Wall -Wextra -Werror -DREDSET_ENABLE_MPI $(INC) ../tests/adapter/adapter_test.c \
	  ../integration/redset_hip_backend.c -o $@ -L$(LIBDIR) -lredset_hip_mpi -lredset_hip $(MPI_HOME)/lib/libmpi.so \
	  -Wl,-rpath,'$$ORIGIN/../../redset_amd/lib:/usr/lib/x86_64-linux-gnu:$(MPI_HOME)/lib'
clean:
	rm -f _ref/adapter_test
.PHONY: all clean
