// cns_hostbuf.h — the host buffers the accept stage returns its results in (cns_hostbuf.hip), and the handle that owns one until it is
// handed to the caller.  No HIP in this header.
#pragma once
#include <stddef.h>

#include <memory>

#include "mecat_hip.h"

// a string buffer of at least `bytes`: the parked one when it fits, else new, touched on `num_threads` threads and page-locked
char* strbuf_get(size_t bytes, int num_threads);
// a result buffer that the copy engine fills (the tables of a batch: 5 bytes per template base): page-locked from 64 MB on, plain
// malloc below; never parked — mhip_cns_free unregisters and frees it
void* result_alloc(size_t bytes, int num_threads);

// owns a buffer that mhip_cns_free releases: one of the two above, or plain malloc
struct CnsFree { void operator()(void* p) const { mhip_cns_free(p); } };
template <typename T> using CnsBuf = std::unique_ptr<T, CnsFree>;
