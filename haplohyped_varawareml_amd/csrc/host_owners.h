// host_owners.h — what a host-side early return must not leak: the file descriptors, mappings and zlib states of the reader
// (reader.hip) and of the ingest engine's source thread (ingest.hip).  Each holder's own code is the only place its resource
// is released, and none can be copied.  Host only, no HIP.
#pragma once
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <zlib.h>

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
struct Fd : NoCopy {
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};
struct Mapping : NoCopy {   // a file mapped read-only
    const uint8_t *p = nullptr;
    size_t len = 0;
    ~Mapping() { if (p) munmap(const_cast<uint8_t *>(p), len); }
};
struct Inflater : NoCopy {   // host zlib, raw DEFLATE: one BGZF member per call
    z_stream zs;
    Inflater()
    {
        memset(&zs, 0, sizeof(zs));
        inflateInit2(&zs, -15);
    }
    ~Inflater() { inflateEnd(&zs); }
    bool member(const uint8_t *src, uint32_t n_in, uint8_t *dst, uint32_t n_out)
    {
        if (inflateReset(&zs) != Z_OK) return false;
        zs.next_in = const_cast<Bytef *>(src);
        zs.avail_in = n_in;
        zs.next_out = dst;
        zs.avail_out = n_out;
        return inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.avail_out == 0;
    }
};
struct GzipInflater : NoCopy {   // host zlib, gzip framing, streaming: begin() per gzip member, end() behind its trailer
    z_stream zs;
    bool open = false;
    ~GzipInflater() { end(); }
    bool begin()
    {
        memset(&zs, 0, sizeof(zs));
        open = inflateInit2(&zs, 15 + 32) == Z_OK;
        return open;
    }
    void end()
    {
        if (open) inflateEnd(&zs);
        open = false;
    }
};
