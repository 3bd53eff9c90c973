/*
 * What the stand-alone host programs of tests/c/ share: the launch stub's counters (tests/stubs/hip_stub.c), one line per check, fake
 * device addresses, and what a refused call has to look like.  One translation unit per program: `failed` is the program's own.
 */
#ifndef GPD_TESTS_HOST_CHECK_H
#define GPD_TESTS_HOST_CHECK_H
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gpd.h"

int hipstub_launches(void);
void hipstub_last(unsigned out[7]);
const char* hipstub_last_kernel(void);
#define KERNEL(piece) (strstr(hipstub_last_kernel(), piece) != NULL)

static int failed;
#define CHECK(cond, what) do { if (!(cond)) { ++failed; printf("FAIL %s (line %d): %s\n", what, __LINE__, gpd_last_error()); } else printf("ok   %s\n", what); } while (0)
#define DEV(n) ((void*)(uintptr_t)(0x100000000ull + 0x1000000ull * (n)))      /* fake device addresses */
#define ODD(p, bytes) ((float*)((char*)(p) + (bytes)))

/* a rejected call: the code, "<entry>:" at the head of the message and the reason in it, nothing launched */
static inline int refused(int rc, int code, const char* entry, const char* reason, int launches_before) {
    return rc == code && strncmp(gpd_last_error(), entry, strlen(entry)) == 0 && gpd_last_error()[strlen(entry)] == ':' &&
           strstr(gpd_last_error(), reason) != NULL && hipstub_launches() == launches_before;
}
#endif
