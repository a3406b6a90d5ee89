# TEST-ONLY: ASan + UBSan build of the PNG read's chunk walk (__host__ __device__, host-only compile:
# no device code, no GPU sanitizer). A makefile of its own beside Makefile, whose `all` is what
# tests/test_sanitizers.py builds; tests/test_png_read_san.py runs `make -f pngd.mk pngd_san`.
# Each -fsanitize= goes after -Xarch_host.
HIPCC   ?= /opt/rocm/bin/hipcc

pngd_san: pngd_san.cpp ../../imagecodecs_amd/csrc/icx_pngd_core.h ../../imagecodecs_amd/csrc/icx_jpeg.h
	$(HIPCC) -x hip --offload-host-only -std=c++17 -fno-strict-aliasing -g -O1 -fno-omit-frame-pointer \
	  -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=all \
	  -o $@ pngd_san.cpp

clean:
	rm -f pngd_san

.PHONY: clean
