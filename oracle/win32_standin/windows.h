// windows.h -- TEST INFRASTRUCTURE: a stand-in for the slice of Win32 / MSVC's CRT that the reference's
// host classes (CArk, CDtaFile, CUtils, CSettings) touch, so that they compile unmodified with g++ into
// oracle/_ref/ref_host (oracle/Makefile, target `ref`).  Force-included in front of every reference TU,
// which is why it also pulls in the standard headers MSVC's own headers drag in for them.
// Nothing of the product includes this; nothing here is taken from the reference.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <strings.h>
#include <sys/stat.h>
#include <sys/types.h>

// MSVC's sized integer keywords (used as `unsigned __int64`, so they have to be macros)
#define __int64 long long
#define _int64 long long

typedef void* HANDLE;
typedef unsigned int DWORD;
typedef int errno_t;
#define MAX_PATH 260
#define INVALID_HANDLE_VALUE ( (HANDLE)-1 )
#define FILE_ATTRIBUTE_DIRECTORY 0x10u
#define FILE_ATTRIBUTE_NORMAL 0x80u

struct WIN32_FIND_DATAA
{
    DWORD dwFileAttributes;
    char cFileName[ MAX_PATH ];
};

// Enumerate `<dir>/<pattern>`; see win32_standin.cpp for the order and what the pattern means.
HANDLE FindFirstFileA( const char* lpPattern, WIN32_FIND_DATAA* lpFindData );
int FindNextFileA( HANDLE lHandle, WIN32_FIND_DATAA* lpFindData );
int FindClose( HANDLE lHandle );

// `\` and `/` both separate path components on Windows; these two turn `\` into `/`.
errno_t fopen_s( FILE** lppFile, const char* lpName, const char* lpMode );
int _mkdir( const char* lpPath );

// memcpy_s: copies nothing when the count exceeds the destination size (the CRT's invalid-parameter
// handler would fire there; the reference never reaches it)
inline errno_t memcpy_s( void* lpDest, size_t lDestSize, const void* lpSrc, size_t lCount )
{
    if( lCount > lDestSize ) return ERANGE;
    memcpy( lpDest, lpSrc, lCount );
    return 0;
}

// _itoa_s: the array-reference template overload of the CRT, radix 10 is all the reference asks for
template < size_t N > inline errno_t _itoa_s( int liValue, char ( &lacBuffer )[ N ], int /*radix*/ )
{
    snprintf( lacBuffer, N, "%d", liValue );
    return 0;
}

// _stricmp: byte-wise, ASCII letters folded to lower case, result by unsigned char -- what the CRT does in the
// "C" locale, and what strcasecmp does there too.
inline int _stricmp( const char* lpA, const char* lpB ) { return strcasecmp( lpA, lpB ); }
